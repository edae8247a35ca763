// Kernel modulation (AdAM's rank-constrained KML) of the frozen filters on the flat parameter buffers — include/rick_hip.h "KML".
//     s[o,i] = sum_r a[o,r] b[i,r]        W^[o,i,t] = W0[o,i,t] (1 + s[o,i])        P[o,i] = sum_t G[o,i,t] W0[o,i,t]
//     da[o,r] = sum_i P[o,i] b[i,r]       db[i,r] = sum_{flagged o} P[o,i] a[o,r]
// over the FLAGGED rows of every layer of a network in one launch each, driven by a device-resident layer table and the compacted
// list of flagged rows (rick_amd/kml.py builds both once per set_rows).  8 B per modulated element in either direction (W0 read,
// W^ written; G and W0 read), P never leaves the registers.  No atomics: every output element has one writer, every sum a fixed
// order, so the results are bit-identical from run to run.
#include "common.h"

#define KML_THREADS 256
#define KML_MAX_RANK 8

// How the 256 threads of a block share the rows of a group — a function of the layer's shape and of the 16-byte phase alone.
// A unit is what one thread takes of a row in one go: four consecutive i (4 taps floats = taps aligned float4) in the vector
// form, one i (taps floats, one by one) otherwise.  `lanes` threads (a power of two) stride over the U units of a row, and
// 256 / lanes rows (slots) are in flight at once.
struct kml_plan {
    int vec, U, lanes, slots;
};

__host__ __device__ __forceinline__ kml_plan kml_make_plan(int ci, int taps, int64_t off, bool phase_ok) {
    kml_plan p;
    p.vec = phase_ok && (taps == 1 || taps == 9) && (ci % 4) == 0 && (off % 4) == 0;
    p.U = p.vec ? ci / 4 : ci;
    p.lanes = 1;
    while (p.lanes < p.U && p.lanes < KML_THREADS) p.lanes <<= 1;
    p.slots = KML_THREADS / p.lanes;
    return p;
}

// db accumulators of a block: [slot][r][ci] floats.  slots * ci <= 1024 whenever U < 256, ci otherwise.
__host__ __device__ __forceinline__ int64_t kml_lds_floats(int rank, int max_ci) { return (int64_t)rank * (max_ci > 1024 ? max_ci : 1024); }

__device__ __forceinline__ bool kml_layer_ok(const rick_kml_layer &L, int rank, int64_t n, int64_t nfac, int64_t nrows_total) {
    return L.co > 0 && L.ci > 0 && L.taps > 0 && L.off >= 0 && L.off + (int64_t)L.co * L.ci * L.taps <= n && L.a_off >= 0 &&
           L.a_off + (int64_t)L.co * rank <= nfac && L.b_off >= 0 && L.b_off + (int64_t)L.ci * rank <= nfac && L.rows_off >= 0 &&
           L.nrows >= 0 && (int64_t)L.rows_off + L.nrows <= nrows_total && L.rg > 0;
}

// s = sum_r a[r] b[r]: the first product, then one FMA per further r, in ascending r.
__device__ __forceinline__ float kml_s(const float *__restrict__ a, const float *__restrict__ b, int rank) {
#pragma clang fp contract(off)
    float s = a[0] * b[0];
    for (int r = 1; r < rank; ++r) s = __builtin_fmaf(a[r], b[r], s);
    return s;
}

// ---- apply: W^ = W0 (1 + s) on the flagged rows.  Block (layer, group) owns rows [group rg, min(nrows, (group + 1) rg)) of the
// layer's compacted list; row k of the group goes to slot k % slots.  Three roundings after s: 1 + s, the product.
template <int TAPS>
__device__ __forceinline__ void kml_apply_unit_vec(const float *__restrict__ w0, float *__restrict__ w, const float *__restrict__ ar,
                                                   const float *__restrict__ b4, int rank) {
#pragma clang fp contract(off)
    float m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = 1.f + kml_s(ar, b4 + q * rank, rank);
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        const float4 v = ld_global4(w0 + 4 * q);
        float4 o;
        o.x = v.x * m[(4 * q + 0) / TAPS];
        o.y = v.y * m[(4 * q + 1) / TAPS];
        o.z = v.z * m[(4 * q + 2) / TAPS];
        o.w = v.w * m[(4 * q + 3) / TAPS];
        *reinterpret_cast<float4 *>(w + 4 * q) = o;
    }
}

__global__ __launch_bounds__(KML_THREADS) void kml_apply_kernel(const float *__restrict__ w0, float *__restrict__ w,
                                                                 const float *__restrict__ fac, int rank,
                                                                 const rick_kml_layer *__restrict__ layers, int nlayers,
                                                                 const int32_t *__restrict__ rows, int64_t nrows_total,
                                                                 const int32_t *__restrict__ blocks, int64_t n, int64_t nfac,
                                                                 int phase_ok) {
#pragma clang fp contract(off)
    const int li = blocks[2 * blockIdx.x], grp = blocks[2 * blockIdx.x + 1];
    if (li < 0 || li >= nlayers) return;
    const rick_kml_layer L = layers[li];
    if (!kml_layer_ok(L, rank, n, nfac, nrows_total) || grp < 0) return;
    const kml_plan p = kml_make_plan(L.ci, L.taps, L.off, phase_ok);
    const int first = grp * L.rg, cnt = min(L.rg, L.nrows - first);
    const int slot = threadIdx.x / p.lanes, lane = threadIdx.x % p.lanes;
    const int64_t rowlen = (int64_t)L.ci * L.taps;
    const float *a = fac + L.a_off, *b = fac + L.b_off;
    for (int k = slot; k < cnt; k += p.slots) {
        const int o = rows[L.rows_off + first + k];
        if (o < 0 || o >= L.co) continue;
        const float *ar = a + (int64_t)o * rank;
        const float *w0r = w0 + L.off + o * rowlen;
        float *wr = w + L.off + o * rowlen;
        for (int u = lane; u < p.U; u += p.lanes) {
            if (p.vec) {
                if (L.taps == 9)
                    kml_apply_unit_vec<9>(w0r + 36 * u, wr + 36 * u, ar, b + (int64_t)4 * u * rank, rank);
                else
                    kml_apply_unit_vec<1>(w0r + 4 * u, wr + 4 * u, ar, b + (int64_t)4 * u * rank, rank);
            } else {
                const float m = 1.f + kml_s(ar, b + (int64_t)u * rank, rank);
                for (int t = 0; t < L.taps; ++t) wr[(int64_t)u * L.taps + t] = w0r[(int64_t)u * L.taps + t] * m;
            }
        }
    }
}

// ---- grad: one pass over G and W0 of the flagged rows.  P[o,i] is one chain over the taps (the first product, then FMAs in
// ascending t).  da[o,r]: a thread adds fma(P[o,i], b[i,r], .) over its i in ascending order; the lanes of the row's slot are
// added by the xor butterfly (lanes / 2, ..., 1 inside a wave; with 128 or 256 lanes the waves of the slot in ascending order
// after the full butterfly) — a function of the row and of b alone.  db: the thread that owns i keeps fma(P[o,i], a[o,r], .)
// over the rows of its slot (ascending) in LDS, the slots are added in ascending order at the end and the block writes its
// partial [r][ci].
template <int TAPS>
__device__ __forceinline__ void kml_grad_unit_vec(const float *__restrict__ g, const float *__restrict__ w0, float P[4]) {
#pragma clang fp contract(off)
    float gv[4 * TAPS], wv[4 * TAPS];
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        const float4 x = ld_global4(g + 4 * q), y = ld_global4(w0 + 4 * q);
        gv[4 * q] = x.x, gv[4 * q + 1] = x.y, gv[4 * q + 2] = x.z, gv[4 * q + 3] = x.w;
        wv[4 * q] = y.x, wv[4 * q + 1] = y.y, wv[4 * q + 2] = y.z, wv[4 * q + 3] = y.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float acc = gv[q * TAPS] * wv[q * TAPS];
#pragma unroll
        for (int t = 1; t < TAPS; ++t) acc = __builtin_fmaf(gv[q * TAPS + t], wv[q * TAPS + t], acc);
        P[q] = acc;
    }
}

__global__ __launch_bounds__(KML_THREADS) void kml_grad_kernel(const float *__restrict__ grad, const float *__restrict__ w0,
                                                                const float *__restrict__ fac, float *__restrict__ dfac,
                                                                float *__restrict__ partials, int64_t npart, int rank,
                                                                const rick_kml_layer *__restrict__ layers, int nlayers,
                                                                const int32_t *__restrict__ rows, int64_t nrows_total,
                                                                const int32_t *__restrict__ blocks, int64_t n, int64_t nfac,
                                                                int phase_ok, int max_ci) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float dbl[];      // [slot][r][ci]
    __shared__ float red[4][KML_MAX_RANK];
    const int li = blocks[2 * blockIdx.x], grp = blocks[2 * blockIdx.x + 1];
    if (li < 0 || li >= nlayers) return;
    const rick_kml_layer L = layers[li];
    if (!kml_layer_ok(L, rank, n, nfac, nrows_total) || grp < 0 || grp >= L.ngroups || L.ci > max_ci) return;
    const int64_t pbase = L.part_off + (int64_t)grp * rank * L.ci;
    if (L.part_off < 0 || pbase + (int64_t)rank * L.ci > npart) return;
    const kml_plan p = kml_make_plan(L.ci, L.taps, L.off, phase_ok);
    const int first = grp * L.rg, cnt = min(L.rg, L.nrows - first);
    const int slot = threadIdx.x / p.lanes, lane = threadIdx.x % p.lanes;
    const int ci = L.ci, taps = L.taps;
    const int64_t rowlen = (int64_t)ci * taps;
    const float *a = fac + L.a_off, *b = fac + L.b_off;
    float *da = dfac + L.a_off;
    const int nacc = p.slots * rank * ci;
    for (int j = threadIdx.x; j < nacc; j += KML_THREADS) dbl[j] = 0.f;
    __syncthreads();
    float *mine = dbl + (int64_t)slot * rank * ci;
    for (int k0 = 0; k0 < cnt; k0 += p.slots) {                  // the same trip count in every thread: the barriers below are uniform
        const int k = k0 + slot;
        int o = k < cnt ? rows[L.rows_off + first + k] : -1;
        if (o >= L.co) o = -1;
        float acc[KML_MAX_RANK];
#pragma unroll
        for (int r = 0; r < KML_MAX_RANK; ++r) acc[r] = 0.f;
        if (o >= 0) {
            const float *gr = grad + L.off + o * rowlen, *w0r = w0 + L.off + o * rowlen;
            float ar[KML_MAX_RANK];
#pragma unroll
            for (int r = 0; r < KML_MAX_RANK; ++r) ar[r] = r < rank ? a[(int64_t)o * rank + r] : 0.f;
            for (int u = lane; u < p.U; u += p.lanes) {
                if (p.vec) {
                    float P[4];
                    if (taps == 9)
                        kml_grad_unit_vec<9>(gr + 36 * u, w0r + 36 * u, P);
                    else
                        kml_grad_unit_vec<1>(gr + 4 * u, w0r + 4 * u, P);
                    const float *b4 = b + (int64_t)4 * u * rank;
#pragma unroll
                    for (int r = 0; r < KML_MAX_RANK; ++r) {
                        if (r < rank) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) acc[r] = __builtin_fmaf(P[q], b4[q * rank + r], acc[r]);
                            float4 *d = reinterpret_cast<float4 *>(mine + r * ci + 4 * u);      // ci % 4 == 0: 16-byte aligned
                            float4 v = *d;
                            v.x = __builtin_fmaf(P[0], ar[r], v.x);
                            v.y = __builtin_fmaf(P[1], ar[r], v.y);
                            v.z = __builtin_fmaf(P[2], ar[r], v.z);
                            v.w = __builtin_fmaf(P[3], ar[r], v.w);
                            *d = v;
                        }
                    }
                } else {
                    const float *ge = gr + (int64_t)u * taps, *we = w0r + (int64_t)u * taps;
                    float P = ge[0] * we[0];
                    for (int t = 1; t < taps; ++t) P = __builtin_fmaf(ge[t], we[t], P);
#pragma unroll
                    for (int r = 0; r < KML_MAX_RANK; ++r) {
                        if (r < rank) {
                            acc[r] = __builtin_fmaf(P, b[(int64_t)u * rank + r], acc[r]);
                            mine[r * ci + u] = __builtin_fmaf(P, ar[r], mine[r * ci + u]);
                        }
                    }
                }
            }
        }
        // da[o, :]: the lanes of the slot
#pragma unroll
        for (int r = 0; r < KML_MAX_RANK; ++r) {
            if (r < rank) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
                    if (off < p.lanes) acc[r] += __shfl_xor(acc[r], off, 64);
            }
        }
        if (p.lanes <= 64) {
            if (o >= 0 && lane == 0)
                for (int r = 0; r < rank; ++r) da[(int64_t)o * rank + r] = acc[r];
        } else {                                                  // a slot of two or four waves (lanes is the same for the whole block)
            if ((threadIdx.x & 63) == 0)
                for (int r = 0; r < rank; ++r) red[threadIdx.x >> 6][r] = acc[r];
            __syncthreads();
            if (o >= 0 && lane == 0) {
                const int w0i = threadIdx.x >> 6;
                for (int r = 0; r < rank; ++r) {
                    float v = red[w0i][r] + red[w0i + 1][r];
                    if (p.lanes == 256) v = (v + red[2][r]) + red[3][r];
                    da[(int64_t)o * rank + r] = v;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // the group's partial of db, [r][ci]: slots in ascending order
    const int per = rank * ci;
    for (int j = threadIdx.x; j < per; j += KML_THREADS) {
        float v = dbl[j];
        for (int s = 1; s < p.slots; ++s) v += dbl[(int64_t)s * per + j];
        partials[pbase + j] = v;
    }
}

// ---- finish: db[i, r] = the layer's partials in ascending group order (0 without a flagged row); da[o, :] = 0 on unflagged rows.
// grid (chunks, layers): chunk c covers elements [256 c, 256 c + 256) of the layer's b (as [r][ci]) and of its a.
__global__ __launch_bounds__(KML_THREADS) void kml_finish_kernel(const float *__restrict__ partials, int64_t npart,
                                                                  float *__restrict__ dfac, int64_t nfac,
                                                                  const uint8_t *__restrict__ rowflags, int64_t nflags, int rank,
                                                                  const rick_kml_layer *__restrict__ layers) {
#pragma clang fp contract(off)
    const rick_kml_layer L = layers[blockIdx.y];
    if (L.co <= 0 || L.ci <= 0 || L.a_off < 0 || L.b_off < 0 || L.a_off + (int64_t)L.co * rank > nfac ||
        L.b_off + (int64_t)L.ci * rank > nfac || L.flags_off < 0 || (int64_t)L.flags_off + L.co > nflags || L.ngroups < 0 ||
        L.part_off < 0 || L.part_off + (int64_t)L.ngroups * rank * L.ci > npart)
        return;
    const int64_t j = (int64_t)blockIdx.x * KML_THREADS + threadIdx.x;
    const int64_t per = (int64_t)rank * L.ci;
    if (j < per) {
        float v = 0.f;
        for (int g = 0; g < L.ngroups; ++g) v += partials[L.part_off + g * per + j];
        const int r = (int)(j / L.ci), i = (int)(j % L.ci);
        dfac[L.b_off + (int64_t)i * rank + r] = v;
    }
    if (j < (int64_t)L.co * rank && !rowflags[L.flags_off + j / rank]) dfac[L.a_off + j] = 0.f;
}

extern "C" int rick_kml_rows_per_group(int ci, int taps) {
    if (ci <= 0 || taps <= 0) return -1;
    // about 16 K elements (64 KB per stream) per block, 4 ... 64 rows: the db partial a group writes (rank x ci floats) stays a
    // small fraction of what it reads (2 x rows x ci x taps)
    const int64_t rg = cdiv64(16384, (int64_t)ci * taps);
    return (int)(rg < 4 ? 4 : rg > 64 ? 64 : rg);
}

static bool kml_common_bad(const void *layers, int nlayers, const void *rows, int64_t nrows_total, const void *blocks, int nblocks,
                           int rank, int64_t n, int64_t nfac) {
    return !layers || nlayers <= 0 || nrows_total < 0 || nblocks < 0 || rank < 1 || rank > KML_MAX_RANK || n < 0 || nfac < 0 ||
           ((uintptr_t)layers % 8) || (nblocks > 0 && (!rows || !blocks || ((uintptr_t)rows % 4) || ((uintptr_t)blocks % 4)));
}

extern "C" int rick_kml_apply_f32(const float *w0, float *w, int64_t n, const float *fac, int64_t nfac, int rank,
                                  const rick_kml_layer *layers, int nlayers, const int32_t *rows, int64_t nrows_total,
                                  const int32_t *blocks, int nblocks, void *stream) {
    if (!w0 || !w || !fac || kml_common_bad(layers, nlayers, rows, nrows_total, blocks, nblocks, rank, n, nfac)) return RICK_EINVAL;
    if ((((uintptr_t)w0 | (uintptr_t)w | (uintptr_t)fac) % 4) || w0 == w) return RICK_EINVAL;
    if (nblocks == 0) return 0;
    const int phase_ok = (uintptr_t)w0 % 16 == 0 && (uintptr_t)w % 16 == 0;
    hipLaunchKernelGGL(kml_apply_kernel, dim3((unsigned)nblocks), dim3(KML_THREADS), 0, (hipStream_t)stream, w0, w, fac, rank, layers,
                       nlayers, rows, nrows_total, blocks, n, nfac, phase_ok);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_kml_grad_f32(const float *grad, const float *w0, int64_t n, const float *fac, float *dfac, int64_t nfac,
                                 float *partials, int64_t npart, int rank, const rick_kml_layer *layers, int nlayers,
                                 const int32_t *rows, int64_t nrows_total, const int32_t *blocks, int nblocks, int max_ci,
                                 void *stream) {
    if (!grad || !w0 || !fac || !dfac || kml_common_bad(layers, nlayers, rows, nrows_total, blocks, nblocks, rank, n, nfac))
        return RICK_EINVAL;
    if ((((uintptr_t)grad | (uintptr_t)w0 | (uintptr_t)fac | (uintptr_t)dfac | (uintptr_t)partials) % 4) || fac == dfac || npart < 0 ||
        max_ci < 1)
        return RICK_EINVAL;
    const int64_t lds = kml_lds_floats(rank, max_ci) * 4;
    if (lds > 64 * 1024) return RICK_EINVAL;                     // ci <= 2048 at rank 8
    if (nblocks == 0) return 0;
    if (!partials) return RICK_EINVAL;
    const int phase_ok = (uintptr_t)grad % 16 == 0 && (uintptr_t)w0 % 16 == 0;
    hipLaunchKernelGGL(kml_grad_kernel, dim3((unsigned)nblocks), dim3(KML_THREADS), (size_t)lds, (hipStream_t)stream, grad, w0, fac,
                       dfac, partials, npart, rank, layers, nlayers, rows, nrows_total, blocks, n, nfac, phase_ok, max_ci);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_kml_grad_finish_f32(const float *partials, int64_t npart, float *dfac, int64_t nfac, const uint8_t *rowflags,
                                        int64_t nflags, int rank, const rick_kml_layer *layers, int nlayers, int max_co, int max_ci,
                                        void *stream) {
    if (!dfac || !rowflags || !layers || nlayers <= 0 || nlayers > 65535 || rank < 1 || rank > KML_MAX_RANK || npart < 0 || nfac < 0 ||
        nflags < 0 || max_co < 1 || max_ci < 1 || (npart > 0 && !partials))
        return RICK_EINVAL;
    if ((((uintptr_t)partials | (uintptr_t)dfac) % 4) || ((uintptr_t)layers % 8)) return RICK_EINVAL;
    const int64_t span = (int64_t)rank * (max_co > max_ci ? max_co : max_ci);
    hipLaunchKernelGGL(kml_finish_kernel, dim3((unsigned)cdiv64(span, KML_THREADS), (unsigned)nlayers), dim3(KML_THREADS), 0,
                       (hipStream_t)stream, partials, npart, dfac, nfac, rowflags, nflags, rank, layers);
    RICK_LAUNCH_STATUS();
}
