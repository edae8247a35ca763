// Gram matrix of a few very long rows and its adjoint — include/rick_hip.h "Gram".  The device side of the cross-domain
// distance-consistency loss (rick_amd/cdc.py): the cosine similarity of whole generator feature maps between the members of a
// batch needs G = X X^T of B <= 8 rows of up to 128 * 1024^2 floats, and its backward pass the row mix dX = (gG + gG^T) X.
// Both kernels stream every row once.  A row is an unordered bag of n values: any memory layout, as long as all rows share it.
// No atomics: every output element has one writer and a fixed summation order.
// The second half of the file is the two-operand form behind the dual contrastive losses (rick_amd/dcl.py): the cross-Gram
// C = A B^T of two row sets in separate allocations with both sets' squared norms from the same pass, and its adjoint.
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

// ==== cross-Gram of two row sets: C[i][j] = <a_i, b_j>, na[i] = <a_i, a_i>, nb[j] = <b_j, b_j> — include/rick_hip.h "Gram" ====
// The first stage is gram_kernel's with two operands: the same slices (gr_slice_len), the same element -> thread map, one fp32 FMA
// chain per product in the same order, the same butterfly and wave order; the slices are added ascending in fp64.  Every entry is
// therefore bit-identical to the entry rick_gram_f32 produces for the same two rows.
// Instantiated for row counts rounded up to 1, 2, 4, 8 (16 size pairs x 2 load paths instead of 64 x 2); the live counts Ba, Bb
// are runtime arguments.  A dead row (index >= the live count) reads the operand's last live row again — an address the wave has
// just requested — and its sums are never written: no load outside the operands, no branch in the loop.
template <int BA, int BB>
struct XgShape {
    static constexpr int NC = BA * BB, NT = BA * BB + BA + BB;       // chains: C row-major, then na, then nb
};

template <int B, bool VEC>
__device__ __forceinline__ void xg_load(float4 (&v)[B], const float *__restrict__ x, int live, int64_t n, int64_t t, int64_t t1) {
#pragma unroll
    for (int i = 0; i < B; i++) {
        const float *r = x + (int64_t)(i < live ? i : live - 1) * n + t;
        if (VEC) {
            v[i] = *reinterpret_cast<const float4 *>(r);
        } else {
            v[i].x = r[0];
            v[i].y = t + 1 < t1 ? r[1] : 0.f;
            v[i].z = t + 2 < t1 ? r[2] : 0.f;
            v[i].w = t + 3 < t1 ? r[3] : 0.f;
        }
    }
}

#define XG_CHAIN(ACC, U, V)              \
    do {                                 \
        ACC = fmaf(U.x, V.x, ACC);       \
        ACC = fmaf(U.y, V.y, ACC);       \
        ACC = fmaf(U.z, V.z, ACC);       \
        ACC = fmaf(U.w, V.w, ACC);       \
    } while (0)

// part[slice][p], p over the LIVE products: i Bb + j, then Ba Bb + i, then Ba Bb + Ba + j.
template <int BA, int BB, bool VEC>
__global__ __launch_bounds__(256) void xgram_kernel(const float *__restrict__ a, int Ba, const float *__restrict__ b, int Bb,
                                                    int64_t n, int64_t slice_len, float *__restrict__ part) {
    constexpr int NC = XgShape<BA, BB>::NC, NT = XgShape<BA, BB>::NT;
    __shared__ float red[4][NT];
    float acc[NT];
#pragma unroll
    for (int p = 0; p < NT; p++) acc[p] = 0.f;
    const int64_t t0 = (int64_t)blockIdx.x * slice_len, t1 = min(n, t0 + slice_len);
#pragma unroll 2
    for (int64_t t = t0 + 4 * (int64_t)threadIdx.x; t < t1; t += 1024) {
        float4 u[BA], v[BB];
        xg_load<BA, VEC>(u, a, Ba, n, t, t1);
        xg_load<BB, VEC>(v, b, Bb, n, t, t1);
#pragma unroll
        for (int i = 0; i < BA; i++)
#pragma unroll
            for (int j = 0; j < BB; j++) XG_CHAIN(acc[i * BB + j], u[i], v[j]);
#pragma unroll
        for (int i = 0; i < BA; i++) XG_CHAIN(acc[NC + i], u[i], u[i]);
#pragma unroll
        for (int j = 0; j < BB; j++) XG_CHAIN(acc[NC + BA + j], v[j], v[j]);
    }
#pragma unroll
    for (int p = 0; p < NT; p++) acc[p] = wave_sum(acc[p]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int p = 0; p < NT; p++) red[threadIdx.x >> 6][p] = acc[p];
    }
    __syncthreads();
    const int live = Ba * Bb + Ba + Bb, p = threadIdx.x;
    if (p < live) {
        int q;                                                       // the chain of live product p
        if (p < Ba * Bb)
            q = (p / Bb) * BB + p % Bb;
        else if (p < Ba * Bb + Ba)
            q = NC + (p - Ba * Bb);
        else
            q = NC + BA + (p - Ba * Bb - Ba);
        part[(int64_t)blockIdx.x * live + p] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// Second stage, as gram_finish_kernel: one 64-lane block per product, slices added ascending in fp64, one writer per output.
__global__ __launch_bounds__(64) void xgram_finish_kernel(const float *__restrict__ part, int nslices, int Ba, int Bb,
                                                          double *__restrict__ C, double *__restrict__ na, double *__restrict__ nb) {
    __shared__ float buf[GR_MAX_SLICES];
    const int live = Ba * Bb + Ba + Bb, p = blockIdx.x;
#pragma unroll 16
    for (int k = threadIdx.x; k < nslices; k += 64) buf[k] = part[(int64_t)k * live + p];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < nslices; k++) s += (double)buf[k];
    if (p < Ba * Bb)
        C[p] = s;
    else if (p < Ba * Bb + Ba)
        na[p - Ba * Bb] = s;
    else
        nb[p - Ba * Bb - Ba] = s;
}

// ---- the adjoint: y[k][t] = d[k] a[k][t] + sum_m M[k][m] b[m][t], one fp32 chain d[k] a[k] -> fma(M[k][0], b[0], .) -> ... ------
// M (Ba x Bb) and d (Ba), device memory, are read once into registers (zero beyond the live counts).  Rows beyond the live counts
// are skipped under wave-uniform conditions: no load, no FMA (a 0 * inf would otherwise reach a live element), no store.
template <int BA, int BB, bool VEC>
__global__ __launch_bounds__(256) void xrowmix_kernel(const float *__restrict__ M, const float *__restrict__ d,
                                                      const float *__restrict__ a, const float *__restrict__ b,
                                                      float *__restrict__ y, int Ba, int Bb, int64_t n) {
    float m[BA * BB], dk[BA];
#pragma unroll
    for (int k = 0; k < BA; k++) {
        dk[k] = k < Ba ? d[k] : 0.f;
#pragma unroll
        for (int q = 0; q < BB; q++) m[k * BB + q] = (k < Ba && q < Bb) ? M[k * Bb + q] : 0.f;
    }
    const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int64_t groups = n >> 2;
        for (int64_t g = first; g < groups; g += step) {
            float4 v[BB];
#pragma unroll
            for (int q = 0; q < BB; q++)
                if (q < Bb) v[q] = *reinterpret_cast<const float4 *>(b + (int64_t)q * n + 4 * g);
#pragma unroll
            for (int k = 0; k < BA; k++) {
                if (k >= Ba) break;
                const float4 u = *reinterpret_cast<const float4 *>(a + (int64_t)k * n + 4 * g);
                float4 o = make_float4(dk[k] * u.x, dk[k] * u.y, dk[k] * u.z, dk[k] * u.w);
#pragma unroll
                for (int q = 0; q < BB; q++)
                    if (q < Bb) {
                        o.x = fmaf(m[k * BB + q], v[q].x, o.x);
                        o.y = fmaf(m[k * BB + q], v[q].y, o.y);
                        o.z = fmaf(m[k * BB + q], v[q].z, o.z);
                        o.w = fmaf(m[k * BB + q], v[q].w, o.w);
                    }
                *reinterpret_cast<float4 *>(y + (int64_t)k * n + 4 * g) = o;
            }
        }
    } else {
        for (int64_t t = first; t < n; t += step) {
            float v[BB];
#pragma unroll
            for (int q = 0; q < BB; q++)
                if (q < Bb) v[q] = b[(int64_t)q * n + t];
#pragma unroll
            for (int k = 0; k < BA; k++) {
                if (k >= Ba) break;
                float o = dk[k] * a[(int64_t)k * n + t];
#pragma unroll
                for (int q = 0; q < BB; q++)
                    if (q < Bb) o = fmaf(m[k * BB + q], v[q], o);
                y[(int64_t)k * n + t] = o;
            }
        }
    }
}

static inline int xg_round(int B) { return B <= 1 ? 1 : B <= 2 ? 2 : B <= 4 ? 4 : 8; }

// LAUNCH(BA, BB) for the rounded-up pair
#define XG_DISPATCH_B(BA_, Bb_, LAUNCH)   \
    switch (xg_round(Bb_)) {              \
        case 1: LAUNCH(BA_, 1); break;    \
        case 2: LAUNCH(BA_, 2); break;    \
        case 4: LAUNCH(BA_, 4); break;    \
        default: LAUNCH(BA_, 8); break;   \
    }
#define XG_DISPATCH(Ba_, Bb_, LAUNCH)                      \
    switch (xg_round(Ba_)) {                               \
        case 1: XG_DISPATCH_B(1, Bb_, LAUNCH) break;       \
        case 2: XG_DISPATCH_B(2, Bb_, LAUNCH) break;       \
        case 4: XG_DISPATCH_B(4, Bb_, LAUNCH) break;       \
        default: XG_DISPATCH_B(8, Bb_, LAUNCH) break;      \
    }

extern "C" int64_t rick_xgram_workspace_bytes(int Ba, int Bb, int64_t n) {
    if (Ba < 1 || Ba > GR_MAXB || Bb < 1 || Bb > GR_MAXB || n < 1) return -1;
    return gr_nslices(n) * (Ba * Bb + Ba + Bb) * (int64_t)sizeof(float);
}

extern "C" int rick_xgram_f32(const float *a, int Ba, const float *b, int Bb, int64_t n, void *ws, double *C, double *na,
                              double *nb, void *stream) {
    if (!a || !b || !ws || !C || !na || !nb || Ba < 1 || Ba > GR_MAXB || Bb < 1 || Bb > GR_MAXB || n < 1 ||
        (((uintptr_t)a | (uintptr_t)b | (uintptr_t)ws) % 4) || (((uintptr_t)C | (uintptr_t)na | (uintptr_t)nb) % 8))
        return RICK_EINVAL;
    const int64_t slice_len = gr_slice_len(n), nslices = gr_nslices(n);
    const bool vec = (((uintptr_t)a | (uintptr_t)b) % 16) == 0 && (n & 3) == 0;      // both operands, or neither
    float *part = (float *)ws;
#define XG_LAUNCH(BA, BB)                                                                                                    \
    do {                                                                                                                     \
        if (vec)                                                                                                             \
            hipLaunchKernelGGL((xgram_kernel<BA, BB, true>), dim3((unsigned)nslices), dim3(256), 0, (hipStream_t)stream, a,  \
                               Ba, b, Bb, n, slice_len, part);                                                               \
        else                                                                                                                 \
            hipLaunchKernelGGL((xgram_kernel<BA, BB, false>), dim3((unsigned)nslices), dim3(256), 0, (hipStream_t)stream, a, \
                               Ba, b, Bb, n, slice_len, part);                                                               \
    } while (0)
    XG_DISPATCH(Ba, Bb, XG_LAUNCH)
#undef XG_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(xgram_finish_kernel, dim3(Ba * Bb + Ba + Bb), dim3(64), 0, (hipStream_t)stream, part, (int)nslices, Ba, Bb,
                       C, na, nb);
    RICK_LAUNCH_STATUS();
}

static inline bool xg_overlap(const float *p, int64_t np, const float *q, int64_t nq) {
    return (uintptr_t)p < (uintptr_t)(q + nq) && (uintptr_t)q < (uintptr_t)(p + np);
}

extern "C" int rick_xrowmix_f32(const float *M, const float *d, const float *a, const float *b, float *y, int Ba, int Bb, int64_t n,
                                void *stream) {
    if (!M || !d || !a || !b || !y || Ba < 1 || Ba > GR_MAXB || Bb < 1 || Bb > GR_MAXB || n < 1 ||
        (((uintptr_t)M | (uintptr_t)d | (uintptr_t)a | (uintptr_t)b | (uintptr_t)y) % 4))
        return RICK_EINVAL;
    if (xg_overlap(y, Ba * n, a, Ba * n) || xg_overlap(y, Ba * n, b, Bb * n)) return RICK_EINVAL;      // y aliases an input
    const bool vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) % 16) == 0 && (n & 3) == 0;
    const int64_t items = vec ? n >> 2 : n;
    const unsigned blocks = cdiv64(items, 256) < GR_MIX_BLOCKS ? (unsigned)cdiv64(items, 256) : GR_MIX_BLOCKS;     // grid-stride
#define XG_LAUNCH(BA, BB)                                                                                                      \
    do {                                                                                                                       \
        if (vec)                                                                                                               \
            hipLaunchKernelGGL((xrowmix_kernel<BA, BB, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, M, d, a, b, y, \
                               Ba, Bb, n);                                                                                     \
        else                                                                                                                   \
            hipLaunchKernelGGL((xrowmix_kernel<BA, BB, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, M, d, a, b,   \
                               y, Ba, Bb, n);                                                                                  \
    } while (0)
    XG_DISPATCH(Ba, Bb, XG_LAUNCH)
#undef XG_LAUNCH
    RICK_LAUNCH_STATUS();
}
