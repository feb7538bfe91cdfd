// The skeleton shared by the residual quantizers that work in a few projected dimensions, csrc/fsq.hip (LD = 8) and csrc/lfq.hip (LD = 16):
//
//     z = W_in x + b_in            W_in [D][dim_g]       project_in
//     zsum = chain(z)              per dimension, the quantizer's own
//     out = W_out zsum + b_out     W_out [dim_g][D]      project_out
//
// and its backward, proj_bwd, which takes the quantizer's (g_z, z) -> (dz, zsum) step as a functor.  fp32 tensors, no float atomics: every output is
// one fixed-order chain, bitwise reproducible run to run.  D = the projected width, LD = the lanes (and LDS entries) a row takes in the chain phases
// (D padded to a power of two), VEC = 16-byte accesses (the launcher's pq_check decides).
//
// Shape of the kernels: a workgroup of 4 waves takes a tile of PQ_ROWS = 16 rows.  (1) the D dot products over dim_g: wave w owns rows 4 w .. 4 w + 3,
// a lane 16-byte pieces of x and W_in, one wave-64 shuffle reduction per (row, j), in DOUBLE (the fp32 products are exact, so z is the float64 dot
// product; fsq.hip says why the chains need that); (2) the chain: the dimensions are independent of each other, so thread (r, j) runs dimension j of
// row r in registers; (3) out: a lane holds W_out for 4 columns in registers and writes a 16-byte piece per row.  x is read once, out written once.
//
// backward (straight-through rounding and the detach() in the residual update leave only the direct path):
//     g_z = W_out^T g_out ;  dz = the functor's ;  dx = W_in^T dz
//     dW_in = dz^T x, db_in = sum dz, dW_out = g_out^T zsum, db_out = sum g_out
// The chain is recomputed from the saved z.  A workgroup takes a chunk of rows (tiles of 16), a thread 4 columns of every per-column quantity, and
// leaves its partial parameter gradients in the caller's workspace; a second launch (proj_bwd_reduce) adds the chunks in chunk order.
#pragma once
#include <initializer_list>

#include "common.hpp"

namespace {

constexpr int PQ_ROWS = 16;                                        // rows per tile
constexpr int PQ_MAX_DIM = 1024, PQ_MAX_Q = 32;                    // dim_g <= 256 threads x 4 columns; Q layers

// 4 floats at p[c .. c + 3]; VEC: c < n, n % 4 == 0 and p 16-byte aligned are the launcher's business
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, int c, int n) {
    if constexpr (VEC) {
        return *reinterpret_cast<const float4*>(p + c);
    } else {
        float4 v;
        v.x = c < n ? p[c] : 0.f;
        v.y = c + 1 < n ? p[c + 1] : 0.f;
        v.z = c + 2 < n ? p[c + 2] : 0.f;
        v.w = c + 3 < n ? p[c + 3] : 0.f;
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void st4(float* __restrict__ p, int c, int n, float4 v) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(p + c) = v;
    } else {
        if (c < n) p[c] = v.x;
        if (c + 1 < n) p[c + 1] = v.y;
        if (c + 2 < n) p[c + 2] = v.z;
        if (c + 3 < n) p[c + 3] = v.w;
    }
}

// w[cc * D + j] = W [n][D] at row c + cc (0 past row n): the 4 D consecutive floats behind W + c D
template <int D, bool VEC>
__device__ __forceinline__ void ld_cols(const float* __restrict__ W, int c, int n, float (&w)[4 * D]) {
    if constexpr (VEC) {
        const float4* p = reinterpret_cast<const float4*>(W + (long long)c * D);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float4 v = p[i];
            w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4 * D; ++e) w[e] = c + e / D < n ? W[(long long)c * D + e] : 0.f;
    }
}

template <int D, bool VEC>
__device__ __forceinline__ void st_cols(float* __restrict__ W, int c, int n, const float (&w)[4 * D]) {
    if constexpr (VEC) {
        float4* p = reinterpret_cast<float4*>(W + (long long)c * D);
#pragma unroll
        for (int i = 0; i < D; ++i) p[i] = make_float4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4 * D; ++e)
            if (c + e / D < n) W[(long long)c * D + e] = w[e];
    }
}

// zl [PQ_ROWS][LD] in LDS = W_in x + b_in of the tile's rows (nothing where there is no row): wave w takes rows 4 w .. 4 w + 3, a lane 4 columns of
// every 256; the caller synchronises
template <int D, bool VEC, int LD>
__device__ __forceinline__ void project_in(const float* __restrict__ x, long long ldx, const float* __restrict__ W_in, const float* __restrict__ b_in,
                                           double* zl, long long row0, int M, int dim_g) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[4][D];                                              // fp32 products are exact in double: z is the float64 dot product
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int j = 0; j < D; ++j) acc[rr][j] = 0.0;
    for (int c = lane * 4; c < dim_g; c += 256) {
        float4 w[D];
#pragma unroll
        for (int j = 0; j < D; ++j) w[j] = ld4<VEC>(W_in + (long long)j * dim_g, c, dim_g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const long long row = row0 + wave * 4 + rr;
            if (row < M) {
                const float4 xv = ld4<VEC>(x + row * ldx, c, dim_g);
#pragma unroll
                for (int j = 0; j < D; ++j)
                    acc[rr][j] = fma((double)xv.w, (double)w[j].w, fma((double)xv.z, (double)w[j].z,
                                     fma((double)xv.y, (double)w[j].y, fma((double)xv.x, (double)w[j].x, acc[rr][j]))));
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double v = wave_sum_d(acc[rr][j]);
            if (lane == rr * D + j) zl[(wave * 4 + rr) * LD + j] = v + (double)b_in[j];
        }
}

// out rows of the tile = W_out zs + b_out, zs [PQ_ROWS][LD] in LDS: wave w takes rows 4 w .. 4 w + 3, a lane 4 columns of every 256
template <int D, bool VEC, int LD>
__device__ __forceinline__ void project_out(const float* zs, const float* __restrict__ W_out, const float* __restrict__ b_out, float* __restrict__ out,
                                            long long ldo, long long row0, int M, int dim_g) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = lane * 4; c < dim_g; c += 256) {
        float w[4 * D];
        ld_cols<D, VEC>(W_out, c, dim_g, w);
        const float4 b = ld4<VEC>(b_out, c, dim_g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = wave * 4 + rr;
            const long long row = row0 + r;
            if (row < M) {
                float4 o = b;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const float zj = zs[r * LD + j];
                    o.x = fmaf(w[j], zj, o.x);
                    o.y = fmaf(w[D + j], zj, o.y);
                    o.z = fmaf(w[2 * D + j], zj, o.z);
                    o.w = fmaf(w[3 * D + j], zj, o.w);
                }
                st4<VEC>(out + row * ldo, c, dim_g, o);
            }
        }
    }
}

// The body of a backward kernel: grid = row chunks (`chunk` rows each, a multiple of 16), 256 threads; partials ws [chunk][epad]: dW_in [D][dim_g] |
// dW_out [dim_g][D] | db_out [dim_g] | db_in [D].  mid(row, j, g_z[j], zsum&) returns dz[j] of the row and leaves zsum[j] of its chain.
template <int D, bool VEC, int LD, class MID>
__device__ __forceinline__ void proj_bwd(const float* __restrict__ g, long long ldg, const float* __restrict__ x, long long ldx,
                                         const float* __restrict__ W_in, const float* __restrict__ W_out, float* __restrict__ dx, long long ldd,
                                         float* __restrict__ ws, int M, int dim_g, int chunk, long long epad, MID mid) {
    __shared__ float gz[PQ_ROWS * LD], dzl[PQ_ROWS * LD], zsl[PQ_ROWS * LD];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = threadIdx.x * 4;                                 // this thread's columns in the per-column part (dim_g <= 1024 = 256 x 4)
    const bool own = c < dim_g;
    float4 wi[D], a_wi[D];
    float a_wo[4 * D];
    float4 a_bo = make_float4(0.f, 0.f, 0.f, 0.f);
    float a_bi = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        wi[j] = own ? ld4<VEC>(W_in + (long long)j * dim_g, c, dim_g) : make_float4(0.f, 0.f, 0.f, 0.f);
        a_wi[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int e = 0; e < 4 * D; ++e) a_wo[e] = 0.f;
    const long long r_begin = (long long)blockIdx.x * chunk;
    const long long r_end = r_begin + chunk < M ? r_begin + chunk : M;
    for (long long row0 = r_begin; row0 < r_end; row0 += PQ_ROWS) {
        {                                                          // g_z = W_out^T g_out: wave <-> 4 rows, lane <-> 4 columns of every 256
            float acc[4][D];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                for (int j = 0; j < D; ++j) acc[rr][j] = 0.f;
            for (int cc = lane * 4; cc < dim_g; cc += 256) {
                float w[4 * D];
                ld_cols<D, VEC>(W_out, cc, dim_g, w);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const long long row = row0 + wave * 4 + rr;
                    if (row < r_end) {
                        const float4 gv = ld4<VEC>(g + row * ldg, cc, dim_g);
#pragma unroll
                        for (int j = 0; j < D; ++j)
                            acc[rr][j] = fmaf(gv.w, w[3 * D + j], fmaf(gv.z, w[2 * D + j], fmaf(gv.y, w[D + j], fmaf(gv.x, w[j], acc[rr][j]))));
                    }
                }
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const float v = wave_sum(acc[rr][j]);
                    if (lane == rr * D + j) gz[(wave * 4 + rr) * LD + j] = v;
                }
        }
        __syncthreads();
        if (PQ_ROWS * LD == 256 || threadIdx.x < PQ_ROWS * LD) {  // thread <-> (row, j): dz and zsum, 0 where there is no row
            const int r = threadIdx.x / LD, j = threadIdx.x % LD;
            const long long row = row0 + r;
            float dzv = 0.f, zsv = 0.f;
            if (j < D && row < r_end) dzv = mid(row, j, gz[r * LD + j], zsv);
            dzl[threadIdx.x] = dzv;
            zsl[threadIdx.x] = zsv;
        }
        __syncthreads();
        if (own) {
            for (int r = 0; r < PQ_ROWS; ++r) {
                const long long row = row0 + r;
                if (row >= r_end) break;
                const float4 xv = ld4<VEC>(x + row * ldx, c, dim_g), gv = ld4<VEC>(g + row * ldg, c, dim_g);
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const float dzj = dzl[r * LD + j], zsj = zsl[r * LD + j];
                    d.x = fmaf(dzj, wi[j].x, d.x), d.y = fmaf(dzj, wi[j].y, d.y), d.z = fmaf(dzj, wi[j].z, d.z), d.w = fmaf(dzj, wi[j].w, d.w);
                    a_wi[j].x = fmaf(dzj, xv.x, a_wi[j].x), a_wi[j].y = fmaf(dzj, xv.y, a_wi[j].y);
                    a_wi[j].z = fmaf(dzj, xv.z, a_wi[j].z), a_wi[j].w = fmaf(dzj, xv.w, a_wi[j].w);
                    a_wo[j] = fmaf(gv.x, zsj, a_wo[j]), a_wo[D + j] = fmaf(gv.y, zsj, a_wo[D + j]);
                    a_wo[2 * D + j] = fmaf(gv.z, zsj, a_wo[2 * D + j]), a_wo[3 * D + j] = fmaf(gv.w, zsj, a_wo[3 * D + j]);
                }
                a_bo.x += gv.x, a_bo.y += gv.y, a_bo.z += gv.z, a_bo.w += gv.w;
                st4<VEC>(dx + row * ldd, c, dim_g, d);
            }
        }
        if (threadIdx.x < D)
            for (int r = 0; r < PQ_ROWS; ++r) a_bi += dzl[r * LD + threadIdx.x];
        __syncthreads();
    }
    float* p = ws + (long long)blockIdx.x * epad;
    const long long n_w = (long long)D * dim_g;
    if (own) {
#pragma unroll
        for (int j = 0; j < D; ++j) st4<VEC>(p + (long long)j * dim_g, c, dim_g, a_wi[j]);
        st_cols<D, VEC>(p + n_w, c, dim_g, a_wo);
        st4<VEC>(p + 2 * n_w, c, dim_g, a_bo);
    }
    if (threadIdx.x < D) p[2 * n_w + dim_g + threadIdx.x] = a_bi;
}

// The body of a reduce kernel, 64 threads: thread <-> one element of (dW_in | dW_out | db_out | db_in), the chunks' partials in chunk order
__device__ __forceinline__ void proj_bwd_reduce(const float* __restrict__ ws, float* __restrict__ dW_in, float* __restrict__ db_in,
                                                float* __restrict__ dW_out, float* __restrict__ db_out, long long n_w, int dim_g, int d, long long epad,
                                                int NC) {
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= 2 * n_w + dim_g + d) return;
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < NC; ++i) s += ws[(long long)i * epad + e];
    if (e < n_w) dW_in[e] = s;
    else if (e < 2 * n_w) dW_out[e - n_w] = s;
    else if (e < 2 * n_w + dim_g) db_out[e - 2 * n_w] = s;
    else db_in[e - 2 * n_w - dim_g] = s;
}

// ---- host side

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// floats of one chunk's partial parameter gradients, and the backward's chunking: 32 rows, doubled until there are at most 1024 chunks
inline long long pq_epad(int dim_g, int d) { return up4(2LL * d * dim_g + dim_g + d); }
inline int pq_chunk(int M) { return row_chunk(M, 32, 1024); }

inline bool pq_in_limits(int dim_g, int d, int Q, int max_d) { return d <= max_d && dim_g <= PQ_MAX_DIM && Q <= PQ_MAX_Q; }

struct PqRows {                                                    // an fp32 [M][dim_g] argument
    const void* p;
    long long ld;
};

// What every launcher checks.  ok: its own argument conditions; layer in [layer_lo, layer_hi]; rows: each present with ld >= dim_g; then the limits;
// weights: the projection parameters the call reads, all null (identity, which needs dim_g == d) or none.  Returns 0 or the error code; vec = every
// row, its leading dimension and every pointer of `aligned` allow 16-byte accesses (meaningless in the identity case).
inline int pq_check(bool ok, int M, int dim_g, int d, int Q, int max_d, int layer_lo, int layer, int layer_hi, std::initializer_list<PqRows> rows,
                    std::initializer_list<const void*> weights, std::initializer_list<const void*> aligned, bool& identity, bool& vec) {
    if (!ok || M <= 0 || dim_g <= 0 || d <= 0 || Q <= 0 || layer < layer_lo || layer > layer_hi) return ALM_ERR_BAD_ARG;
    for (const PqRows& r : rows)
        if (!r.p || r.ld < dim_g) return ALM_ERR_BAD_ARG;
    if (!pq_in_limits(dim_g, d, Q, max_d)) return ALM_ERR_UNSUPPORTED;
    size_t absent = 0;
    for (const void* w : weights) absent += !w;
    identity = absent == weights.size();
    if (identity ? dim_g != d : absent != 0) return ALM_ERR_BAD_ARG;
    vec = dim_g % 4 == 0;
    for (const PqRows& r : rows) vec = vec && r.ld % 4 == 0 && al16(r.p);
    for (const void* p : aligned) vec = vec && al16(p);
    return 0;
}

// CALL(N) with N = d, for d = 1 .. MAX_D (8 <= MAX_D <= 10); wider d never gets here (pq_check)
#define ALM_PQ_D(MAX_D, CALL)                            \
    switch (d) {                                         \
        case 1: CALL(1); break;                          \
        case 2: CALL(2); break;                          \
        case 3: CALL(3); break;                          \
        case 4: CALL(4); break;                          \
        case 5: CALL(5); break;                          \
        case 6: CALL(6); break;                          \
        case 7: CALL(7); break;                          \
        case 8: CALL(8); break;                          \
        case 9: CALL((MAX_D < 9 ? MAX_D : 9)); break;    \
        default: CALL(MAX_D); break;                     \
    }

}  // namespace
