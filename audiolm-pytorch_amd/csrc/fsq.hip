// Residual finite scalar quantization (FSQ, arXiv 2309.15505 Appendix A, in the residual form of vector-quantize-pytorch's ResidualFSQ; restated in
// tests/fsq_restated.py) for gfx950, forward, decode and backward, fp32, no float atomics (every output is one fixed-order chain, bitwise
// reproducible run to run).  Per group, levels L (d entries), Q layers, k = last active layer:
//
//     z = W_in x + b_in                                       W_in [d][dim_g]   (identity when dim_g == d: no weights at all)
//     r_0 = z ;  for q in 0..k:  t_q = tanh(r_q / scale_q + shift) ;  c_q = rint(t_q half_l - offset)
//                                idx_q = sum_j (c_q[j] + half_w[j]) basis[j] ;  quant_q = c_q / half_w * scale_q ;  r_{q+1} = r_q - quant_q
//     zsum = sum_q quant_q ;  out = W_out zsum + b_out        W_out [dim_g][d]
//
// Every per-level constant comes from the caller's table (computed in double on the host, rounded once to fp32): no atanh / pow here.
//
// Precision.  All tensors are fp32, but z and the chain are carried in DOUBLE: layer q divides the residual by scale_q = (L - 1)^-q, so an absolute
// error e of z becomes an error e (L - 1)^q of the tanh argument -- with fp32 z (e ~ 1e-6 after a 512-term dot product) and L = 8 that is
// order 1 at q = 7, i.e. the codes of the deep layers and the (1 - t^2) terms of the backward would be functions of rounding noise.  In double the
// dot product of fp32 inputs is exact to 1e-16, z - quant is carried without loss and scale_q is formed by repeated division, so the indices are
// those of float64 arithmetic on the same fp32 inputs.  The table's half_l / offset / shift enter the bound unamplified (1e-7 relative); its
// scale / (1 / scale) rows serve the decode, whose sum has no such amplification.  The saved z [M][d] is double for the same reason.
//
// Shape of the kernels: a workgroup of 4 waves takes a tile of 16 rows.  (1) the d dot products over dim_g: wave w owns rows 4 w .. 4 w + 3, a lane
// 16-byte pieces of x and W_in, one wave-64 shuffle reduction per (row, j); (2) the chain: the dimensions are independent of each other, so thread
// (r, j) of the first 128 runs dimension j of row r in registers and the layer's index is a 3-step shuffle sum over the 8 lanes of a row; (3) out:
// a lane holds W_out for 4 columns in registers and writes a 16-byte piece per row.  x is read once, out written once.
//
// backward (the detach() in the residual update leaves only the direct path):
//     g_z = W_out^T g_out ;  dz = g_z * sum_{q <= k} (half_l / half_w) (1 - t_q^2) ;  dx = W_in^T dz
//     dW_in = dz^T x, db_in = sum dz, dW_out = g_out^T zsum, db_out = sum g_out
// The chain is recomputed from the saved z.  A workgroup takes a chunk of rows (tiles of 16), a thread 4 columns of every per-column quantity, and
// leaves its partial parameter gradients in the caller's workspace; a second launch adds the chunks in chunk order.
#include "common.hpp"
#include "../../include/audiolm_hip.h"

namespace {

constexpr int FSQ_MAX_D = 8, FSQ_MAX_DIM = 1024, FSQ_MAX_Q = 32;
constexpr int FSQ_ROWS = 16;                                       // rows per tile
// rows of the constant table (8 floats each), then scale [Q][8] and 1 / scale [Q][8]
constexpr int C_HALF_L = 0, C_OFFSET = 8, C_SHIFT = 16, C_INV_HALF_W = 24, C_HALF_W = 32, C_BASIS = 40, C_LEVELS = 48, C_SCALE = 56;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

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

// The forward chain of dimension j of one row, called by ALL lanes of a wave (lane = 8 r + j within the wave's 8 rows; `active` = j < D and the
// row exists).  Returns zsum[j]; writes the row's indices (idx_row = idx + row * ldi, Q columns, -1 past k) with lane j storing columns j, j + 8, ..
template <int D>
__device__ __forceinline__ float chain_fwd(double res, bool active, int j, const float* __restrict__ consts, int Q, int k, long long* __restrict__ idx_row) {
    const int jj = j < D ? j : 0;
    const double half_l = consts[C_HALF_L + jj], offset = consts[C_OFFSET + jj], shift = consts[C_SHIFT + jj];
    const double half_w = consts[C_HALF_W + jj], lm1 = (double)consts[C_LEVELS + jj] - 1.0;
    const int basis = (int)consts[C_BASIS + jj];
    double zsum = 0.0, sc = 1.0;                                   // sc = (L - 1)^-q by repeated division
    int mine[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        mine[qq] = -1;
        for (int q8 = 0; q8 < 8; ++q8) {
            const int q = qq * 8 + q8;
            if (q > k) break;                                      // wave-uniform
            const double t = tanh(res / sc + shift);
            const double c = rint(t * half_l - offset);            // round half to even
            int code = active ? (int)(c + half_w) * basis : 0;
            code += __shfl_xor(code, 1, 64);
            code += __shfl_xor(code, 2, 64);
            code += __shfl_xor(code, 4, 64);
            if (q8 == j) mine[qq] = code;
            const double quant = c / half_w * sc;
            zsum += quant;
            res -= quant;
            sc /= lm1;
        }
    }
    if (idx_row) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
            if (qq * 8 + j < Q) idx_row[qq * 8 + j] = (long long)mine[qq];
    }
    return (float)zsum;
}

// the backward's chain: returns sum_{q <= k} (half_l / half_w) (1 - t_q^2) and leaves zsum[j] in `zsum`
template <int D>
__device__ __forceinline__ float chain_bwd(double res, int j, const float* __restrict__ consts, int k, float& zsum) {
    const double half_l = consts[C_HALF_L + j], offset = consts[C_OFFSET + j], shift = consts[C_SHIFT + j];
    const double half_w = consts[C_HALF_W + j], lm1 = (double)consts[C_LEVELS + j] - 1.0;
    double s = 0.0, zs = 0.0, sc = 1.0;
    for (int q = 0; q <= k; ++q) {
        const double t = tanh(res / sc + shift);
        s += 1.0 - t * t;
        const double quant = rint(t * half_l - offset) / half_w * sc;
        zs += quant;
        res -= quant;
        sc /= lm1;
    }
    zsum = (float)zs;
    return (float)(s * (half_l / half_w));
}

// zsum[j] of one row from its code indices (columns 0 .. ncols - 1 of idx_row; a negative entry contributes nothing)
__device__ __forceinline__ float codes_to_zsum(const long long* __restrict__ idx_row, int ncols, int j, const float* __restrict__ consts) {
    const float inv_hw = consts[C_INV_HALF_W + j];
    const int half_w = (int)consts[C_HALF_W + j], levels = (int)consts[C_LEVELS + j];
    const long long basis = (long long)consts[C_BASIS + j];
    float zs = 0.f;
    for (int q = 0; q < ncols; ++q) {
        const long long id = idx_row[q];
        if (id < 0) continue;
        const int c = (int)((id / basis) % levels) - half_w;
        zs += (float)c * inv_hw * consts[C_SCALE + 8 * q + j];
    }
    return zs;
}

// out rows of the tile = W_out zs + b_out, zs [FSQ_ROWS][8] in LDS: wave w takes rows 4 w .. 4 w + 3, a lane 4 columns of every 256
template <int D, bool VEC>
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
                    const float zj = zs[r * 8 + j];
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

// grid ceil(M / 16), 256 threads
template <int D, bool VEC>
__global__ __launch_bounds__(256) void fsq_fwd_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ W_in,
                                                      const float* __restrict__ b_in, const float* __restrict__ W_out, const float* __restrict__ b_out,
                                                      const float* __restrict__ consts, long long* __restrict__ idx, long long ldi,
                                                      float* __restrict__ out, long long ldo, double* __restrict__ z_out, int M, int dim_g, int Q, int k) {
    __shared__ double zl[FSQ_ROWS * 8];
    __shared__ float zs[FSQ_ROWS * 8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row0 = (long long)blockIdx.x * FSQ_ROWS;
    {
        double acc[4][D];                                          // fp32 products are exact in double: z is the float64 dot product
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
                if (lane == rr * D + j) zl[(wave * 4 + rr) * 8 + j] = v + (double)b_in[j];
            }
    }
    __syncthreads();
    if (threadIdx.x < FSQ_ROWS * 8) {
        const int r = threadIdx.x >> 3, j = threadIdx.x & 7;
        const long long row = row0 + r;
        const bool active = j < D && row < M;
        const double zv = zl[r * 8 + (j < D ? j : 0)];
        if (z_out && active) z_out[row * D + j] = zv;
        const float zsum = chain_fwd<D>(zv, active, j, consts, Q, k, row < M ? idx + row * ldi : nullptr);
        if (j < D) zs[r * 8 + j] = zsum;
    }
    __syncthreads();
    project_out<D, VEC>(zs, W_out, b_out, out, ldo, row0, M, dim_g);
}

// dim_g == d, no projections: thread <-> (row, j), 32 rows per workgroup
template <int D>
__global__ __launch_bounds__(256) void fsq_fwd_identity_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ consts,
                                                               long long* __restrict__ idx, long long ldi, float* __restrict__ out, long long ldo,
                                                               double* __restrict__ z_out, int M, int Q, int k) {
    const int j = threadIdx.x & 7;
    const long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool active = j < D && row < M;
    const double zv = active ? (double)x[row * ldx + j] : 0.0;
    if (z_out && active) z_out[row * D + j] = zv;
    const float zsum = chain_fwd<D>(zv, active, j, consts, Q, k, row < M ? idx + row * ldi : nullptr);
    if (active) out[row * ldo + j] = zsum;
}

template <int D, bool VEC>
__global__ __launch_bounds__(256) void fsq_decode_kernel(const long long* __restrict__ idx, long long ldi, const float* __restrict__ W_out,
                                                         const float* __restrict__ b_out, const float* __restrict__ consts, float* __restrict__ out,
                                                         long long ldo, int M, int dim_g, int ncols) {
    __shared__ float zs[FSQ_ROWS * 8];
    const long long row0 = (long long)blockIdx.x * FSQ_ROWS;
    if (threadIdx.x < FSQ_ROWS * 8) {
        const int r = threadIdx.x >> 3, j = threadIdx.x & 7;
        const long long row = row0 + r;
        if (j < D) zs[r * 8 + j] = row < M ? codes_to_zsum(idx + row * ldi, ncols, j, consts) : 0.f;
    }
    __syncthreads();
    project_out<D, VEC>(zs, W_out, b_out, out, ldo, row0, M, dim_g);
}

template <int D>
__global__ __launch_bounds__(256) void fsq_decode_identity_kernel(const long long* __restrict__ idx, long long ldi, const float* __restrict__ consts,
                                                                  float* __restrict__ out, long long ldo, int M, int ncols) {
    const int j = threadIdx.x & 7;
    const long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (j < D && row < M) out[row * ldo + j] = codes_to_zsum(idx + row * ldi, ncols, j, consts);
}

// grid = row chunks (`chunk` rows each, a multiple of 16), 256 threads; partials ws [chunk][epad]: dW_in [D][dim_g] | dW_out [dim_g][D] | db_out
// [dim_g] | db_in [D]
template <int D, bool VEC>
__global__ __launch_bounds__(256) void fsq_bwd_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ x, long long ldx,
                                                      const double* __restrict__ z, const float* __restrict__ W_in, const float* __restrict__ W_out,
                                                      const float* __restrict__ consts, float* __restrict__ dx, long long ldd, float* __restrict__ ws,
                                                      int M, int dim_g, int Q, int k, int chunk, long long epad) {
    __shared__ float gz[FSQ_ROWS * 8], dzl[FSQ_ROWS * 8], zsl[FSQ_ROWS * 8];
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
    for (long long row0 = r_begin; row0 < r_end; row0 += FSQ_ROWS) {
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
                    if (lane == rr * D + j) gz[(wave * 4 + rr) * 8 + j] = v;
                }
        }
        __syncthreads();
        if (threadIdx.x < FSQ_ROWS * 8) {                          // thread <-> (row, j): dz and zsum, 0 where there is no row
            const int r = threadIdx.x >> 3, j = threadIdx.x & 7;
            const long long row = row0 + r;
            float dzv = 0.f, zsv = 0.f;
            if (j < D && row < r_end) dzv = gz[r * 8 + j] * chain_bwd<D>(z[row * D + j], j, consts, k, zsv);
            dzl[threadIdx.x] = dzv;
            zsl[threadIdx.x] = zsv;
        }
        __syncthreads();
        if (own) {
            for (int r = 0; r < FSQ_ROWS; ++r) {
                const long long row = row0 + r;
                if (row >= r_end) break;
                const float4 xv = ld4<VEC>(x + row * ldx, c, dim_g), gv = ld4<VEC>(g + row * ldg, c, dim_g);
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const float dzj = dzl[r * 8 + j], zsj = zsl[r * 8 + j];
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
            for (int r = 0; r < FSQ_ROWS; ++r) a_bi += dzl[r * 8 + threadIdx.x];
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

// thread <-> one element of (dW_in | dW_out | db_out | db_in): the chunks' partials in chunk order
__global__ __launch_bounds__(64) void fsq_bwd_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW_in, float* __restrict__ db_in,
                                                            float* __restrict__ dW_out, float* __restrict__ db_out, long long n_w, int dim_g, int d,
                                                            long long epad, int NC) {
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

template <int D>
__global__ __launch_bounds__(256) void fsq_bwd_identity_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ x, long long ldx,
                                                               const float* __restrict__ consts, float* __restrict__ dx, long long ldd, int M, int Q,
                                                               int k) {
    const int j = threadIdx.x & 7;
    const long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (j < D && row < M) {
        float zsum;
        dx[row * ldd + j] = g[row * ldg + j] * chain_bwd<D>((double)x[row * ldx + j], j, consts, k, zsum);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline long long up4(long long n) { return (n + 3) & ~3LL; }
inline long long fsq_epad(int dim_g, int d) { return up4(2LL * d * dim_g + dim_g + d); }

inline int fsq_chunk(int M) {
    int ch = 32;
    while ((M + ch - 1) / ch > 1024) ch *= 2;
    return ch;
}

inline bool fsq_in_limits(int dim_g, int d, int Q) { return d <= FSQ_MAX_D && dim_g <= FSQ_MAX_DIM && Q <= FSQ_MAX_Q; }

#define ALM_FSQ_D(CALL)           \
    switch (d) {                  \
        case 1: CALL(1); break;   \
        case 2: CALL(2); break;   \
        case 3: CALL(3); break;   \
        case 4: CALL(4); break;   \
        case 5: CALL(5); break;   \
        case 6: CALL(6); break;   \
        case 7: CALL(7); break;   \
        default: CALL(8); break;  \
    }

}  // namespace

// floats of the constant table of Q layers: 7 rows of 8 (half_l, offset, shift, 1 / half_w, half_w, basis, levels), then scale [Q][8], 1 / scale [Q][8]
extern "C" int alm_fsq_consts_floats(int Q) { return Q < 1 || Q > FSQ_MAX_Q ? -1 : C_SCALE + 16 * Q; }

extern "C" int alm_fsq_fwd(const float* x, long long ldx, const float* W_in, const float* b_in, const float* W_out, const float* b_out,
                           const float* consts, long long* idx, long long ldi, float* out, long long ldo, double* z, int M, int dim_g, int d, int Q, int k,
                           void* stream) {
    if (M <= 0 || dim_g <= 0 || d <= 0 || Q <= 0 || k < 0 || k >= Q || !x || !consts || !idx || !out || ldx < dim_g || ldo < dim_g || ldi < Q)
        return ALM_ERR_BAD_ARG;
    if (!fsq_in_limits(dim_g, d, Q)) return ALM_ERR_UNSUPPORTED;
    const bool identity = !W_in && !b_in && !W_out && !b_out;
    if (identity ? dim_g != d : (!W_in || !b_in || !W_out || !b_out)) return ALM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (identity) {
        const dim3 grid((unsigned)((M + 31) / 32));
#define ALM_CALL(N) hipLaunchKernelGGL((fsq_fwd_identity_kernel<N>), grid, dim3(256), 0, st, x, ldx, consts, idx, ldi, out, ldo, z, M, Q, k)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    } else {
        const dim3 grid((unsigned)((M + FSQ_ROWS - 1) / FSQ_ROWS));
        const bool vec = dim_g % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out) && al16(W_in) && al16(W_out) && al16(b_out);
#define ALM_CALL(N)                                                                                                                                      \
    if (vec) hipLaunchKernelGGL((fsq_fwd_kernel<N, true>), grid, dim3(256), 0, st, x, ldx, W_in, b_in, W_out, b_out, consts, idx, ldi, out, ldo, z, M,  \
                                dim_g, Q, k);                                                                                                            \
    else hipLaunchKernelGGL((fsq_fwd_kernel<N, false>), grid, dim3(256), 0, st, x, ldx, W_in, b_in, W_out, b_out, consts, idx, ldi, out, ldo, z, M,     \
                            dim_g, Q, k)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    }
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_fsq_decode(const long long* idx, long long ldi, const float* W_out, const float* b_out, const float* consts, float* out,
                              long long ldo, int M, int dim_g, int d, int Q, int ncols, void* stream) {
    if (M <= 0 || dim_g <= 0 || d <= 0 || Q <= 0 || ncols <= 0 || ncols > Q || !idx || !consts || !out || ldo < dim_g || ldi < ncols) return ALM_ERR_BAD_ARG;
    if (!fsq_in_limits(dim_g, d, Q)) return ALM_ERR_UNSUPPORTED;
    const bool identity = !W_out && !b_out;
    if (identity ? dim_g != d : (!W_out || !b_out)) return ALM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (identity) {
        const dim3 grid((unsigned)((M + 31) / 32));
#define ALM_CALL(N) hipLaunchKernelGGL((fsq_decode_identity_kernel<N>), grid, dim3(256), 0, st, idx, ldi, consts, out, ldo, M, ncols)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    } else {
        const dim3 grid((unsigned)((M + FSQ_ROWS - 1) / FSQ_ROWS));
        const bool vec = dim_g % 4 == 0 && ldo % 4 == 0 && al16(out) && al16(W_out) && al16(b_out);
#define ALM_CALL(N)                                                                                                                     \
    if (vec) hipLaunchKernelGGL((fsq_decode_kernel<N, true>), grid, dim3(256), 0, st, idx, ldi, W_out, b_out, consts, out, ldo, M, dim_g, ncols); \
    else hipLaunchKernelGGL((fsq_decode_kernel<N, false>), grid, dim3(256), 0, st, idx, ldi, W_out, b_out, consts, out, ldo, M, dim_g, ncols)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    }
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of alm_fsq_bwd: row chunks (32 rows, doubled until there are at most 1024 chunks) x the parameter
// gradients' 2 d dim_g + dim_g + d floats rounded up to 4; 0 in the identity case (dim_g == d: no parameters); -1 outside the limits or past 2^31
extern "C" int alm_fsq_bwd_ws_floats(int M, int dim_g, int d) {
    if (M <= 0 || dim_g <= 0 || d <= 0 || dim_g == d) return 0;
    if (!fsq_in_limits(dim_g, d, 1)) return -1;
    const int ch = fsq_chunk(M);
    const long long n = (long long)((M + ch - 1) / ch) * fsq_epad(dim_g, d);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_fsq_bwd(const float* g, long long ldg, const float* x, long long ldx, const double* z, const float* W_in, const float* W_out,
                           const float* consts, float* dx, long long ldd, float* dW_in, float* db_in, float* dW_out, float* db_out, float* ws,
                           long long ws_floats, int M, int dim_g, int d, int Q, int k, void* stream) {
    if (M <= 0 || dim_g <= 0 || d <= 0 || Q <= 0 || k < 0 || k >= Q || !g || !x || !consts || !dx || ldg < dim_g || ldx < dim_g || ldd < dim_g)
        return ALM_ERR_BAD_ARG;
    if (!fsq_in_limits(dim_g, d, Q)) return ALM_ERR_UNSUPPORTED;
    const bool identity = !W_in && !W_out;
    hipStream_t st = (hipStream_t)stream;
    if (identity) {
        if (dim_g != d) return ALM_ERR_BAD_ARG;
        const dim3 grid((unsigned)((M + 31) / 32));
#define ALM_CALL(N) hipLaunchKernelGGL((fsq_bwd_identity_kernel<N>), grid, dim3(256), 0, st, g, ldg, x, ldx, consts, dx, ldd, M, Q, k)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
        ALM_LAUNCH_CHECK();
        return 0;
    }
    if (!W_in || !W_out || !z || !dW_in || !db_in || !dW_out || !db_out || !ws) return ALM_ERR_BAD_ARG;
    const int ch = fsq_chunk(M), NC = (M + ch - 1) / ch;
    const long long epad = fsq_epad(dim_g, d), need = (long long)NC * epad;
    if (need > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    const bool vec = dim_g % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && ldd % 4 == 0 && al16(g) && al16(x) && al16(dx) && al16(W_in) && al16(W_out) && al16(ws);
#define ALM_CALL(N)                                                                                                                                   \
    if (vec) hipLaunchKernelGGL((fsq_bwd_kernel<N, true>), dim3((unsigned)NC), dim3(256), 0, st, g, ldg, x, ldx, z, W_in, W_out, consts, dx, ldd, ws, \
                                M, dim_g, Q, k, ch, epad);                                                                                            \
    else hipLaunchKernelGGL((fsq_bwd_kernel<N, false>), dim3((unsigned)NC), dim3(256), 0, st, g, ldg, x, ldx, z, W_in, W_out, consts, dx, ldd, ws,    \
                            M, dim_g, Q, k, ch, epad)
    ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    ALM_LAUNCH_CHECK();
    const long long E = 2LL * d * dim_g + dim_g + d;
    hipLaunchKernelGGL(fsq_bwd_reduce_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, st, ws, dW_in, db_in, dW_out, db_out, (long long)d * dim_g,
                       dim_g, d, epad, NC);
    ALM_LAUNCH_CHECK();
    return 0;
}
