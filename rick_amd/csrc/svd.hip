// FSGAN's singular-value adaptation on the flat parameter buffers — include/rick_hip.h "SVD".  A weight is W[co][ci][taps]; per tap
// t the stored fp32 factors U[t][co][r], Vt[t][r][ci] (r = min(co, ci)) of the source weight are frozen and the shift d[t][r] of
// the singular values is learnt:
//     W^[o,i,t] = W0[o,i,t] + sum_k (U[t,o,k] d[t,k]) Vt[t,k,i]          dd[t,k] = sum_o sum_i U[t,o,k] G[o,i,t] Vt[t,k,i]
// for every layer of a network in one launch each, driven by a device-resident layer table and a (layer, tile) list per block
// (rick_amd/svd.py builds both once).  The products run on v_mfma_f32_32x32x2_f32: exact fp32 products, one fp32 fma chain per
// output in ascending k (apply) / ascending o (grad).  No atomics: every output has one writer and every sum an order that is a
// function of the layer's shape alone, so results are bit-identical from run to run, whatever else is in the table and wherever
// the layer lies.  Rows and columns beyond co, ci and r enter as zeros by SELECTION (the address is clamped into the layer, the
// value replaced): nothing is ever read from a neighbouring layer, nothing multiplied by zero to hide it.
#include "common.h"

#define SVD_THREADS 256
#define SVD_MAX_TAPS 16
#define SVD_OC 32                                               // rows of G a grad block stages at a time
#define SVD_KC 16                                               // k per staged chunk of U d in apply
#define SVD_A_LD (SVD_KC + 1)

typedef float svd_f32x16 __attribute__((ext_vector_type(16)));

// A block owns `units` = taps * sub MFMA tiles of 32 x 32, unit un = (tap un / sub, sub-tile un % sub), wave w the units
// w, w + 4, ...: nine taps of one tile, or four sub-tiles of a 1 x 1 / linear weight.  units <= 16.
__host__ __device__ __forceinline__ int svd_sub(int taps) { return taps >= 4 ? 1 : 4 / taps; }
// A value that is outside the layer enters as zero: the load goes to a clamped address INSIDE the layer and is unconditional (a
// select the compiler turns into a branch around the load serialises the loads of a chunk), the value is then kept or replaced.
__device__ __forceinline__ float svd_keep(float v, bool keep) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) & (keep ? 0xffffffffu : 0u));
}
// row of accumulator register `reg` in lane half h (the column is lane & 31)
__device__ __forceinline__ int svd_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---- apply.  Block (layer, tile): rows [o0, o0 + 32) x columns [i0, i0 + 32 sub) of the layer, ALL taps.  A = U d (rounded
// once), B = Vt, K = r ascending, two k per instruction.  U's rows lie r floats apart, so a wave reads its 32 x SVD_KC chunk of U
// along k (four rows of 64 B per load), scales it by d and turns it through a wave-private LDS tile into the fragment order;
// Vt's rows are read as they lie.  The per-tap result tiles go to LDS as [o][(i - i0) taps + t] — the weight's own tap-innermost
// order — and the epilogue adds W0 and stores each row's run of (columns x taps) floats contiguously.
__global__ __launch_bounds__(SVD_THREADS) void svd_apply_kernel(const float *__restrict__ w0, float *__restrict__ w,
                                                                 const float *__restrict__ u, const float *__restrict__ vt,
                                                                 const float *__restrict__ d,
                                                                 const rick_svd_layer *__restrict__ layers, int nlayers,
                                                                 const int32_t *__restrict__ blocks) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][32][SVD_KC + 1] operand tiles, then [32][32 sub taps] results
    const int li = blocks[2 * blockIdx.x], tile = blocks[2 * blockIdx.x + 1];
    if (li < 0 || li >= nlayers) return;
    const rick_svd_layer L = layers[li];
    const int co = L.co, ci = L.ci, taps = L.taps, r = L.r;
    const int sub = svd_sub(taps), iw = 32 * sub, nit = cdiv(ci, iw);
    if (tile < 0 || tile >= nit * cdiv(co, 32)) return;
    const int o0 = (tile / nit) * 32, i0 = (tile % nit) * iw;
    const int ld = iw * taps, units = taps * sub;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
    const int kk = lane & (SVD_KC - 1), rb = lane >> 4;          // staging: column kk of rows rb, rb + 4, ...
    float *aw = lds + wave * (32 * SVD_A_LD), *res = lds + 4 * 32 * SVD_A_LD;
    // every wave runs the same number of unit iterations; a wave without a unit works on zeros and stores nothing
    for (int un0 = 0; un0 < units; un0 += 4) {
        const int un = un0 + wave;
        const bool act = un < units;
        const int t = act ? un / sub : 0, is = act ? un % sub : 0;
        const int i = i0 + is * 32 + l31;
        const bool iok = act && i < ci;
        const float *ut = u + L.u_off + (int64_t)t * co * r;
        const float *dp = d + L.d_off + (int64_t)t * r;
        const float *vp = vt + L.vt_off + (int64_t)t * r * ci + (i < ci ? i : ci - 1);
        svd_f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int k0 = 0; k0 < r; k0 += SVD_KC) {
            float st[8], bv[SVD_KC / 2];
            {
                const int k = k0 + kk;
                const bool kok = act && k < r;
                const int kc = k < r ? k : r - 1;
                const float dk = dp[kc];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int o = o0 + rb + 4 * j;
                    const float uu = ut[(int64_t)(o < co ? o : co - 1) * r + kc];
                    st[j] = svd_keep(uu * dk, kok && o < co);
                }
            }
#pragma unroll
            for (int s = 0; s < SVD_KC / 2; ++s) {
                const int k = k0 + 2 * s + h;
                const float vv = vp[(int64_t)(k < r ? k : r - 1) * ci];
                bv[s] = svd_keep(vv, iok && k < r);
            }
            // the tile is private to the wave: wave-scope ordering is all it needs (no block barrier couples the waves, which
            // work on different taps).  The previous chunk's fragment reads were consumed by its MFMAs above.
#pragma unroll
            for (int j = 0; j < 8; ++j) aw[(rb + 4 * j) * SVD_A_LD + kk] = st[j];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int s = 0; s < SVD_KC / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[l31 * SVD_A_LD + 2 * s + h], bv[s], acc, 0, 0, 0);
        }
        if (act) {
#pragma unroll
            for (int q = 0; q < 16; ++q) res[svd_row(q, h) * ld + (is * 32 + l31) * taps + t] = acc[q];
        }
    }
    __syncthreads();
    const int ncols = min(iw, ci - i0) * taps, nrows = min(32, co - o0);
    for (int row = wave; row < nrows; row += 4) {
        const int64_t g = L.off + ((int64_t)(o0 + row) * ci + i0) * taps;
        for (int c = lane; c < ncols; c += 64) w[g + c] = w0[g + c] + res[row * ld + c];
    }
}

// ---- grad.  Block (layer, tile): singular directions [k0, k0 + 32 sub) x columns [i0, i0 + 32) of the layer, ALL taps.  Per
// unit T[k,i] = sum_o U[t,o,k] G[o,i,t] on the MFMA (A = U^T read along k, B = G from LDS, K = o ascending).  G's rows are staged
// SVD_OC at a time as the contiguous run [o][(i - i0) taps + t] they are in memory (row stride 32 taps + 1: odd, so the
// fragment reads — lane stride taps — are conflict-free for odd taps) and serve every tap.  Epilogue: T[k,i] Vt[t,k,i], the 32
// columns added by the 16, 8, 4, 2, 1 xor butterfly, one partial per (t, k, column tile); T is never stored.
__global__ __launch_bounds__(SVD_THREADS) void svd_grad_kernel(const float *__restrict__ grad, const float *__restrict__ u,
                                                                const float *__restrict__ vt, float *__restrict__ partials,
                                                                const rick_svd_layer *__restrict__ layers, int nlayers,
                                                                const int32_t *__restrict__ blocks) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float gs[];   // [SVD_OC][32 taps + 1]
    const int li = blocks[2 * blockIdx.x], tile = blocks[2 * blockIdx.x + 1];
    if (li < 0 || li >= nlayers) return;
    const rick_svd_layer L = layers[li];
    const int co = L.co, ci = L.ci, taps = L.taps, r = L.r;
    const int sub = svd_sub(taps), kw = 32 * sub, nit = cdiv(ci, 32);
    if (tile < 0 || tile >= nit * cdiv(r, kw)) return;
    const int k0 = (tile / nit) * kw, it = tile % nit, i0 = it * 32;
    const int ld = 32 * taps + 1, units = taps * sub;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
    const int icols = min(32, ci - i0) * taps;
    svd_f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
    for (int oc = 0; oc < co; oc += SVD_OC) {
        __syncthreads();
        for (int c = lane; c < 32 * taps; c += 64) {             // a wave takes rows wave, wave + 4, ...: eight loads in flight
            const int cc = c < icols ? c : 0;
            float v[SVD_OC / 4];
#pragma unroll
            for (int j = 0; j < SVD_OC / 4; ++j) {
                const int o = oc + wave + 4 * j;
                v[j] = grad[L.off + ((int64_t)(o < co ? o : co - 1) * ci + i0) * taps + cc];
            }
#pragma unroll
            for (int j = 0; j < SVD_OC / 4; ++j) gs[(wave + 4 * j) * ld + c] = svd_keep(v[j], oc + wave + 4 * j < co && c < icols);
        }
        __syncthreads();
#pragma unroll 1
        for (int ob = 0; ob < SVD_OC; ob += 16) {                // 16 rows = 8 instructions per unit at a time
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int un = wave + 4 * q;
                if (un < units) {
                    const int t = un / sub, k = k0 + (un % sub) * 32 + l31;
                    const bool kok = k < r;
                    const float *up = u + L.u_off + (int64_t)t * co * r + (kok ? k : r - 1);
                    float av[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        const int o = oc + ob + 2 * s + h;
                        const bool ook = o < co;
                        const float uu = up[(int64_t)(ook ? o : co - 1) * r];
                        av[s] = svd_keep(uu, ook && kok);
                    }
#pragma unroll
                    for (int s = 0; s < 8; ++s)
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], gs[(ob + 2 * s + h) * ld + l31 * taps + t], acc[q], 0, 0, 0);
                }
            }
        }
    }
    const int i = i0 + l31;
    const bool iok = i < ci;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int un = wave + 4 * q;
        if (un < units) {
            const int t = un / sub, kb = k0 + (un % sub) * 32;
            const float *vp = vt + L.vt_off + (int64_t)t * r * ci + (iok ? i : ci - 1);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = kb + svd_row(e, h);
                const bool kok = k < r;
                const float vv = vp[(int64_t)(kok ? k : r - 1) * ci];
                float p = acc[q][e] * svd_keep(vv, iok && kok);
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
                if (l31 == 0 && kok) partials[L.part_off + ((int64_t)t * r + k) * nit + it] = p;
            }
        }
    }
}

// ---- finish: dd[t,k] = the column-tile partials of (t, k) in ascending tile order.  grid (chunks, layers), one writer per output.
__global__ __launch_bounds__(SVD_THREADS) void svd_finish_kernel(const float *__restrict__ partials, float *__restrict__ dd,
                                                                  const rick_svd_layer *__restrict__ layers) {
#pragma clang fp contract(off)
    const rick_svd_layer L = layers[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * SVD_THREADS + threadIdx.x;
    if (j >= (int64_t)L.taps * L.r) return;
    const int nit = cdiv(L.ci, 32);
    const float *p = partials + L.part_off + j * nit;
    float v = p[0];
    for (int it = 1; it < nit; ++it) v += p[it];
    dd[L.d_off + j] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int rick_svd_apply_tiles(int co, int ci, int taps) {
    if (co <= 0 || ci <= 0 || taps <= 0 || taps > SVD_MAX_TAPS) return -1;
    const int64_t n = cdiv64(co, 32) * cdiv64(ci, 32 * svd_sub(taps));
    return n > INT32_MAX ? -1 : (int)n;
}

extern "C" int rick_svd_grad_tiles(int co, int ci, int taps) {
    if (co <= 0 || ci <= 0 || taps <= 0 || taps > SVD_MAX_TAPS) return -1;
    const int r = co < ci ? co : ci;
    const int64_t n = cdiv64(r, 32 * svd_sub(taps)) * cdiv64(ci, 32);
    return n > INT32_MAX ? -1 : (int)n;
}

extern "C" int64_t rick_svd_partials(int co, int ci, int taps) {
    if (co <= 0 || ci <= 0 || taps <= 0 || taps > SVD_MAX_TAPS) return -1;
    return (int64_t)taps * (co < ci ? co : ci) * cdiv64(ci, 32);
}

extern "C" int rick_svd_check_table(const rick_svd_layer *layers_host, int nlayers, int64_t n, int64_t nu, int64_t nvt, int64_t nd,
                                    int64_t npart) {
    if (!layers_host || nlayers <= 0 || nlayers > 65535 || n < 0 || nu < 0 || nvt < 0 || nd < 0 || npart < 0) return RICK_EINVAL;
    for (int k = 0; k < nlayers; ++k) {
        const rick_svd_layer &L = layers_host[k];
        if (L.co <= 0 || L.ci <= 0 || L.taps <= 0 || L.taps > SVD_MAX_TAPS || L.r != (L.co < L.ci ? L.co : L.ci)) return RICK_EINVAL;
        const int64_t tr = (int64_t)L.taps * L.r;
        if (L.off < 0 || L.u_off < 0 || L.vt_off < 0 || L.d_off < 0 || L.part_off < 0) return RICK_EINVAL;
        if (L.off > n || (int64_t)L.co * L.ci * L.taps > n - L.off || L.u_off > nu || tr * L.co > nu - L.u_off || L.vt_off > nvt ||
            tr * L.ci > nvt - L.vt_off || L.d_off > nd || tr > nd - L.d_off || L.part_off > npart ||
            tr * cdiv64(L.ci, 32) > npart - L.part_off)
            return RICK_EINVAL;
    }
    return 0;
}

// A pointer the kernels may dereference: known to the runtime as device (or managed) memory.
static bool svd_on_device(const void *p) {
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

static bool svd_tables_bad(const rick_svd_layer *layers, const rick_svd_layer *layers_host, int nlayers, const int32_t *blocks,
                           int nblocks, bool grad) {
    if (!layers || !layers_host || nlayers <= 0 || !blocks || nblocks <= 0 || ((uintptr_t)layers % 8) || ((uintptr_t)blocks % 4))
        return true;
    int64_t tiles = 0;                                          // the block list covers every tile of the table, no more
    for (int k = 0; k < nlayers; ++k) {
        const rick_svd_layer &L = layers_host[k];
        const int t = grad ? rick_svd_grad_tiles(L.co, L.ci, L.taps) : rick_svd_apply_tiles(L.co, L.ci, L.taps);
        if (t < 0) return true;
        tiles += t;
    }
    return tiles != nblocks;
}

extern "C" int rick_svd_apply_f32(const float *w0, float *w, int64_t n, const float *u, int64_t nu, const float *vt, int64_t nvt,
                                  const float *d, int64_t nd, const rick_svd_layer *layers, const rick_svd_layer *layers_host,
                                  int nlayers, const int32_t *blocks, int nblocks, void *stream) {
    if (!w0 || !w || !u || !vt || !d || w0 == w || ((((uintptr_t)w0 | (uintptr_t)w | (uintptr_t)u | (uintptr_t)vt | (uintptr_t)d)) % 4))
        return RICK_EINVAL;
    if (svd_tables_bad(layers, layers_host, nlayers, blocks, nblocks, false)) return RICK_EINVAL;
    if (rick_svd_check_table(layers_host, nlayers, n, nu, nvt, nd, INT64_MAX)) return RICK_EINVAL;
    if (!svd_on_device(w0) || !svd_on_device(w) || !svd_on_device(u) || !svd_on_device(vt) || !svd_on_device(d) ||
        !svd_on_device(layers) || !svd_on_device(blocks))
        return RICK_EINVAL;
    int lds = 0;
    for (int k = 0; k < nlayers; ++k) {
        const int f = 32 * 32 * svd_sub(layers_host[k].taps) * layers_host[k].taps;
        lds = f > lds ? f : lds;
    }
    lds = (lds + 4 * 32 * SVD_A_LD) * 4;
    if (lds > 64 * 1024) RICK_LDS160_ONCE(svd_apply_kernel);     // taps >= 15
    hipLaunchKernelGGL(svd_apply_kernel, dim3((unsigned)nblocks), dim3(SVD_THREADS), (size_t)lds, (hipStream_t)stream, w0, w, u, vt, d,
                       layers, nlayers, blocks);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_svd_grad_f32(const float *grad, int64_t n, const float *u, int64_t nu, const float *vt, int64_t nvt,
                                 float *partials, int64_t npart, const rick_svd_layer *layers, const rick_svd_layer *layers_host,
                                 int nlayers, const int32_t *blocks, int nblocks, void *stream) {
    if (!grad || !u || !vt || !partials || ((((uintptr_t)grad | (uintptr_t)u | (uintptr_t)vt | (uintptr_t)partials)) % 4))
        return RICK_EINVAL;
    if (svd_tables_bad(layers, layers_host, nlayers, blocks, nblocks, true)) return RICK_EINVAL;
    if (rick_svd_check_table(layers_host, nlayers, n, nu, nvt, INT64_MAX, npart)) return RICK_EINVAL;
    if (!svd_on_device(grad) || !svd_on_device(u) || !svd_on_device(vt) || !svd_on_device(partials) || !svd_on_device(layers) ||
        !svd_on_device(blocks))
        return RICK_EINVAL;
    int taps = 1;
    for (int k = 0; k < nlayers; ++k) taps = layers_host[k].taps > taps ? layers_host[k].taps : taps;
    hipLaunchKernelGGL(svd_grad_kernel, dim3((unsigned)nblocks), dim3(SVD_THREADS), (size_t)SVD_OC * (32 * taps + 1) * 4,
                       (hipStream_t)stream, grad, u, vt, partials, layers, nlayers, blocks);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_svd_grad_finish_f32(const float *partials, int64_t npart, float *dd, int64_t nd, const rick_svd_layer *layers,
                                        const rick_svd_layer *layers_host, int nlayers, void *stream) {
    if (!partials || !dd || !layers || ((((uintptr_t)partials | (uintptr_t)dd)) % 4) || ((uintptr_t)layers % 8)) return RICK_EINVAL;
    if (rick_svd_check_table(layers_host, nlayers, INT64_MAX, INT64_MAX, INT64_MAX, nd, npart)) return RICK_EINVAL;
    if (!svd_on_device(partials) || !svd_on_device(dd) || !svd_on_device(layers)) return RICK_EINVAL;
    int64_t span = 1;
    for (int k = 0; k < nlayers; ++k) {
        const int64_t tr = (int64_t)layers_host[k].taps * layers_host[k].r;
        span = tr > span ? tr : span;
    }
    hipLaunchKernelGGL(svd_finish_kernel, dim3((unsigned)cdiv64(span, SVD_THREADS), (unsigned)nlayers), dim3(SVD_THREADS), 0,
                       (hipStream_t)stream, partials, dd, layers);
    RICK_LAUNCH_STATUS();
}
