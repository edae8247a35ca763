// VGG16 fc2 features for on-device improved precision / recall — include/rick_hip.h "VGG16 fc2".
//
// The 13 convolutions of the trunk run on rick_inc_conv_f32 (inception.hip) and the five 2x2 max pools on
// rick_lpips_maxpool2_f32 (lpips.hip).  This file holds what is specific to the fc2 path: the input (nearest resize to
// 224 x 224, no affine) and the two fully connected layers, a skinny GEMM (M <= 64 rows) that streams its weights once.
// No atomics: every output element has one writer and a fixed summation order.
#include "common.h"

// the resize index is floorf of ONE fp32 product, and the reduce stage is a chain of fp32 additions: nothing may be fused
#pragma clang fp contract(off)

typedef float fc_f32x16 __attribute__((ext_vector_type(16)));

#define VGG_SIZE 224

// ---- input: planar [N, 3, H, W] -> nearest resize to 224 x 224 -> NHWC4 (channel 3 = 0) -----------------------------------
// F.interpolate(size=(224, 224)) (mode 'nearest'): src = min(int(floorf(dst * scale)), in - 1), scale = float(in) / float(out)
// in fp32 (computed on the host, one IEEE division).  Values are copied.
__global__ __launch_bounds__(256) void vgg_input_kernel(const float *__restrict__ x, float *__restrict__ out, int N, int H, int W,
                                                        float sh, float sw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * VGG_SIZE * VGG_SIZE) return;
    const int ox = (int)(i % VGG_SIZE), oy = (int)((i / VGG_SIZE) % VGG_SIZE);
    const int64_t n = i / (VGG_SIZE * VGG_SIZE);
    const int iy = min((int)floorf(__fmul_rn((float)oy, sh)), H - 1), ix = min((int)floorf(__fmul_rn((float)ox, sw)), W - 1);
    const float *p = x + n * 3 * H * W + (int64_t)iy * W + ix;
    reinterpret_cast<float4 *>(out)[i] = make_float4(p[0], p[(int64_t)H * W], p[(int64_t)2 * H * W], 0.f);
}

// ---- fully connected layer, stage 1: split-K partials on the f32-input MFMA ------------------------------------------------
// part[s][m][n] = sum over the k of slice s of x[m][k] * W[n][k]  (v_mfma_f32_32x32x2_f32: exact fp32 products, an fp32 fma
// chain in k order).
//
// Packed weights: [Np / 32 column blocks][Kp / 8 k blocks][64 lanes][4], Np = N rounded up to 128, Kp = K rounded up to 8,
// zero padded.  Lane (h = lane >> 5, c = lane & 31) of k block kb holds W[32 nb + c][8 kb + 2 j + h], j = 0..3: one
// global_load_dwordx4 per lane = 1 KiB per wave, contiguous, and its four components are the B operands of four consecutive
// MFMAs.  A wave owns one 32-column block and streams that block's k blocks of its slice front to back.
//
// Block = 4 waves = 128 columns x one K slice x all M rows (MT tiles of 32; rows >= M are zero).  The x tile of a stage
// (FC_CH k blocks = 64 k) is shared through LDS in the same lane layout, so every operand read is one ds_read_b128; the slot
// of lane l in k block kb is rotated by 2 kb lanes, which spreads the staging writes (ds_write_b32, 32 banks) over the banks.
// Stage c + 1's global loads (weights to registers, x to registers -> the other LDS buffer) are in flight while stage c is
// multiplied: 8 KiB of weights per wave.
//
// Summation order of part[s][m][n]: two fp32 fma chains, one over the even and one over the odd k blocks of the slice (counted
// from the slice's first), each in the order k block ascending, j ascending, h = 0 then 1 inside the MFMA; then even + odd.
// Two chains halve the length of the longest one (784 k for fc1) at no cost in MFMA issue.  The order depends on (K, N) alone:
// the slicing (fc_plan) does not look at M, and rows are independent accumulators, so row m is bit-identical whatever M is and
// whatever the other rows hold.
#define FC_BN 128             // columns per block
#define FC_KB 8               // k per packed block
#define FC_CH 8               // k blocks per stage
#define FC_TARGET_BLOCKS 512  // two blocks per CU
#define FC_MIN_SLICE_KB 32    // a slice is at least 256 k (but for the last)

// K slices of a layer: (number of slices, k blocks per slice); a function of (K, N) only
static void fc_plan(int K, int N, int *slices, int *kbs) {
    const int KB = cdiv(K, FC_KB), nbk = cdiv(N, FC_BN);
    int S = cdiv(FC_TARGET_BLOCKS, nbk);
    if (S > KB / FC_MIN_SLICE_KB) S = KB / FC_MIN_SLICE_KB;
    if (S < 1) S = 1;
    *kbs = cdiv(KB, S);
    *slices = cdiv(KB, *kbs);
}

template <int MT>
__global__ __launch_bounds__(256) void fc_partial_kernel(const float *__restrict__ x, const float *__restrict__ wpk,
                                                         float *__restrict__ part, int M, int K, int N, int KB, int kbs, int vec) {
    __shared__ __attribute__((aligned(16))) float xs[2][FC_CH * MT * 256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, h = lane >> 5, l32 = lane & 31;
    const int nb = blockIdx.x * 4 + w, s = blockIdx.y;
    const int kb0 = s * kbs, kb1 = min(KB, kb0 + kbs), nchunks = cdiv(kb1 - kb0, FC_CH);
    const float *wp = wpk + (int64_t)nb * KB * 256 + lane * 4;

    float4 wr[FC_CH], xr[2 * MT];
    // x staging item idx = t + 256 i: row idx >> 4, float4 idx & 15 of the stage's 64 k
#define FC_LOAD(c_)                                                                                                          \
    do {                                                                                                                     \
        const int kbc = kb0 + (c_) * FC_CH;                                                                                  \
        _Pragma("unroll") for (int i = 0; i < 2 * MT; i++) {                                                                 \
            const int idx = t + 256 * i, row = idx >> 4, q4 = idx & 15, k = kbc * FC_KB + 4 * q4;                            \
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                                                                      \
            if (row < M && kbc + (q4 >> 1) < kb1) {                                                                          \
                const float *p = x + (int64_t)row * K + k;                                                                   \
                if (vec) {                                                                                                   \
                    if (k < K) v = *reinterpret_cast<const float4 *>(p);                                                     \
                } else {                                                                                                     \
                    if (k < K) v.x = p[0];                                                                                   \
                    if (k + 1 < K) v.y = p[1];                                                                               \
                    if (k + 2 < K) v.z = p[2];                                                                               \
                    if (k + 3 < K) v.w = p[3];                                                                               \
                }                                                                                                            \
            }                                                                                                                \
            xr[i] = v;                                                                                                       \
        }                                                                                                                    \
        _Pragma("unroll") for (int kb = 0; kb < FC_CH; kb++)                                                                 \
            wr[kb] = kbc + kb < kb1 ? ld_global4(wp + (int64_t)(kbc + kb) * 256) : make_float4(0.f, 0.f, 0.f, 0.f);          \
    } while (0)
    // element i4 of the float4 at (row, q4) is k = 8 kb + 2 j + hh with kb = q4 >> 1, j = 2 (q4 & 1) + (i4 >> 1), hh = i4 & 1
#define FC_STORE(buf_)                                                                                                       \
    do {                                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < 2 * MT; i++) {                                                                 \
            const int idx = t + 256 * i, row = idx >> 4, q4 = idx & 15, kb = q4 >> 1, j = 2 * (q4 & 1);                      \
            float *d = xs[buf_] + (kb * MT + (row >> 5)) * 256;                                                              \
            const int l0 = ((row & 31) + 2 * kb) & 63, l1 = (l0 + 32) & 63;                                                  \
            d[l0 * 4 + j] = xr[i].x;                                                                                         \
            d[l1 * 4 + j] = xr[i].y;                                                                                         \
            d[l0 * 4 + j + 1] = xr[i].z;                                                                                     \
            d[l1 * 4 + j + 1] = xr[i].w;                                                                                     \
        }                                                                                                                    \
    } while (0)

    fc_f32x16 acc[2][MT];                                              // [parity of the k block within the slice]
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[p][mt][e] = 0.f;

    FC_LOAD(0);
    FC_STORE(0);
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
        float4 wc[FC_CH];
#pragma unroll
        for (int kb = 0; kb < FC_CH; kb++) wc[kb] = wr[kb];
        if (c + 1 < nchunks) FC_LOAD(c + 1);
        const float *xb = xs[c & 1];
        const int nk = min(FC_CH, kb1 - kb0 - c * FC_CH);
#pragma unroll
        for (int kb = 0; kb < FC_CH; kb++) {
            if (kb < nk) {                                             // block-uniform
                float4 xv[MT];
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    xv[mt] = *reinterpret_cast<const float4 *>(xb + (kb * MT + mt) * 256 + ((lane + 2 * kb) & 63) * 4);
#pragma unroll
                for (int mt = 0; mt < MT; mt++) {
                    fc_f32x16 &a = acc[kb & 1][mt];                    // FC_CH is even: kb & 1 is the parity within the slice
                    a = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[mt].x, wc[kb].x, a, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[mt].y, wc[kb].y, a, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[mt].z, wc[kb].z, a, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[mt].w, wc[kb].w, a, 0, 0, 0);
                }
            }
        }
        if (c + 1 < nchunks) FC_STORE((c + 1) & 1);
        __syncthreads();
    }
#undef FC_LOAD
#undef FC_STORE

    // D[row = (e & 3) + 8 (e >> 2) + 4 h][col = l32]
    const int n = nb * 32 + l32;
    if (n >= N) return;
    float *dst = part + (int64_t)s * M * N + n;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int m = mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (m < M) dst[(int64_t)m * N] = __fadd_rn(acc[0][mt][e], acc[1][mt][e]);
        }
}

// ---- stage 2: out[m][n] = act(((part[0] + part[1]) + ... + part[S - 1]) + bias[n]), slices in order --------------------------
__global__ __launch_bounds__(256) void fc_reduce_kernel(const float *__restrict__ part, const float *__restrict__ bias,
                                                        float *__restrict__ out, int MN, int N, int S, int relu) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    float v = part[i];
    for (int s = 1; s < S; s++) v = __fadd_rn(v, part[(int64_t)s * MN + i]);
    v = __fadd_rn(v, bias[i % N]);
    out[i] = relu ? fmaxf(v, 0.f) : v;
}

static bool fc_shape_ok(int M, int K, int N) {
    return M >= 1 && M <= 64 && K >= 1 && N >= 1 && K <= (1 << 24) && N <= (1 << 20);
}

extern "C" int rick_vgg_input_f32(const float *x, float *out, int N, int H, int W, void *stream) {
    if (!x || !out || N < 0 || H <= 0 || W <= 0 || ((uintptr_t)out % 16)) return RICK_EINVAL;
    if (N == 0) return 0;
    const int64_t total = (int64_t)N * VGG_SIZE * VGG_SIZE;
    if (cdiv64(total, 256) > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(vgg_input_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, N, H, W,
                       (float)H / (float)VGG_SIZE, (float)W / (float)VGG_SIZE);
    RICK_LAUNCH_STATUS();
}

extern "C" int64_t rick_fc_packed_floats(int K, int N) {
    if (!fc_shape_ok(1, K, N)) return -1;
    return (int64_t)cdiv(N, FC_BN) * FC_BN * cdiv(K, FC_KB) * FC_KB;
}

extern "C" int64_t rick_fc_workspace_floats(int M, int K, int N) {
    if (!fc_shape_ok(M, K, N)) return -1;
    int S, kbs;
    fc_plan(K, N, &S, &kbs);
    return (int64_t)S * M * N;
}

extern "C" int rick_fc_f32(const float *x, const float *wpk, const float *bias, float *ws, float *out, int M, int K, int N,
                           int relu, void *stream) {
    if (!x || !wpk || !bias || !ws || !out || !fc_shape_ok(M, K, N) || ((uintptr_t)wpk % 16)) return RICK_EINVAL;
    int S, kbs;
    fc_plan(K, N, &S, &kbs);
    const int KB = cdiv(K, FC_KB), vec = (K % 4 == 0) && ((uintptr_t)x % 16 == 0);
    const dim3 grid((unsigned)cdiv(N, FC_BN), (unsigned)S);
    if (M <= 32)
        hipLaunchKernelGGL(fc_partial_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, wpk, ws, M, K, N, KB, kbs, vec);
    else
        hipLaunchKernelGGL(fc_partial_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, wpk, ws, M, K, N, KB, kbs, vec);
    hipLaunchKernelGGL(fc_reduce_kernel, dim3((unsigned)cdiv(M * N, 256)), dim3(256), 0, (hipStream_t)stream, ws, bias, out, M * N,
                       N, S, relu);
    RICK_LAUNCH_STATUS();
}
