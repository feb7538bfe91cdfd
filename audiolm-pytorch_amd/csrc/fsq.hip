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
// The projections, the tiling and the whole backward except the chain's derivative are csrc/proj_quant.hpp (LD = 8 lanes per row).  The chain here:
// thread (r, j) of the first 128 runs dimension j of row r in registers and the layer's index is a 3-step shuffle sum over the 8 lanes of a row.
// backward: dz = g_z * sum_{q <= k} (half_l / half_w) (1 - t_q^2), the chain recomputed from the saved z.
#include "proj_quant.hpp"

namespace {

constexpr int FSQ_MAX_D = 8;
constexpr int FSQ_LD = 8;                                          // lanes (and LDS entries) per row in the chain phases
// rows of the constant table (8 floats each), then scale [Q][8] and 1 / scale [Q][8]
constexpr int C_HALF_L = 0, C_OFFSET = 8, C_SHIFT = 16, C_INV_HALF_W = 24, C_HALF_W = 32, C_BASIS = 40, C_LEVELS = 48, C_SCALE = 56;

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

// grid ceil(M / 16), 256 threads
template <int D, bool VEC>
__global__ __launch_bounds__(256) void fsq_fwd_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ W_in,
                                                      const float* __restrict__ b_in, const float* __restrict__ W_out, const float* __restrict__ b_out,
                                                      const float* __restrict__ consts, long long* __restrict__ idx, long long ldi,
                                                      float* __restrict__ out, long long ldo, double* __restrict__ z_out, int M, int dim_g, int Q, int k) {
    __shared__ double zl[PQ_ROWS * FSQ_LD];
    __shared__ float zs[PQ_ROWS * FSQ_LD];
    const long long row0 = (long long)blockIdx.x * PQ_ROWS;
    project_in<D, VEC, FSQ_LD>(x, ldx, W_in, b_in, zl, row0, M, dim_g);
    __syncthreads();
    if (threadIdx.x < PQ_ROWS * FSQ_LD) {
        const int r = threadIdx.x >> 3, j = threadIdx.x & 7;
        const long long row = row0 + r;
        const bool active = j < D && row < M;
        const double zv = zl[r * FSQ_LD + (j < D ? j : 0)];
        if (z_out && active) z_out[row * D + j] = zv;
        const float zsum = chain_fwd<D>(zv, active, j, consts, Q, k, row < M ? idx + row * ldi : nullptr);
        if (j < D) zs[r * FSQ_LD + j] = zsum;
    }
    __syncthreads();
    project_out<D, VEC, FSQ_LD>(zs, W_out, b_out, out, ldo, row0, M, dim_g);
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
    __shared__ float zs[PQ_ROWS * FSQ_LD];
    const long long row0 = (long long)blockIdx.x * PQ_ROWS;
    if (threadIdx.x < PQ_ROWS * FSQ_LD) {
        const int r = threadIdx.x >> 3, j = threadIdx.x & 7;
        const long long row = row0 + r;
        if (j < D) zs[r * FSQ_LD + j] = row < M ? codes_to_zsum(idx + row * ldi, ncols, j, consts) : 0.f;
    }
    __syncthreads();
    project_out<D, VEC, FSQ_LD>(zs, W_out, b_out, out, ldo, row0, M, dim_g);
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
    proj_bwd<D, VEC, FSQ_LD>(g, ldg, x, ldx, W_in, W_out, dx, ldd, ws, M, dim_g, chunk, epad, [=](long long row, int j, float gzj, float& zsum) {
        return gzj * chain_bwd<D>(z[row * D + j], j, consts, k, zsum);
    });
}

__global__ __launch_bounds__(64) void fsq_bwd_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW_in, float* __restrict__ db_in,
                                                            float* __restrict__ dW_out, float* __restrict__ db_out, long long n_w, int dim_g, int d,
                                                            long long epad, int NC) {
    proj_bwd_reduce(ws, dW_in, db_in, dW_out, db_out, n_w, dim_g, d, epad, NC);
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

#define ALM_FSQ_D(CALL) ALM_PQ_D(FSQ_MAX_D, CALL)

}  // namespace

// floats of the constant table of Q layers: 7 rows of 8 (half_l, offset, shift, 1 / half_w, half_w, basis, levels), then scale [Q][8], 1 / scale [Q][8]
extern "C" int alm_fsq_consts_floats(int Q) { return Q < 1 || Q > PQ_MAX_Q ? -1 : C_SCALE + 16 * Q; }

extern "C" int alm_fsq_fwd(const float* x, long long ldx, const float* W_in, const float* b_in, const float* W_out, const float* b_out,
                           const float* consts, long long* idx, long long ldi, float* out, long long ldo, double* z, int M, int dim_g, int d, int Q, int k,
                           void* stream) {
    bool identity, vec;
    if (const int err = pq_check(consts && idx && ldi >= Q, M, dim_g, d, Q, FSQ_MAX_D, 0, k, Q - 1, {{x, ldx}, {out, ldo}}, {W_in, b_in, W_out, b_out},
                                 {W_in, W_out, b_out}, identity, vec))
        return err;
    hipStream_t st = (hipStream_t)stream;
    if (identity) {
        const dim3 grid((unsigned)((M + 31) / 32));
#define ALM_CALL(N) hipLaunchKernelGGL((fsq_fwd_identity_kernel<N>), grid, dim3(256), 0, st, x, ldx, consts, idx, ldi, out, ldo, z, M, Q, k)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    } else {
        const dim3 grid((unsigned)((M + PQ_ROWS - 1) / PQ_ROWS));
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
    bool identity, vec;
    if (const int err = pq_check(idx && consts && ldi >= ncols, M, dim_g, d, Q, FSQ_MAX_D, 1, ncols, Q, {{out, ldo}}, {W_out, b_out}, {W_out, b_out},
                                 identity, vec))
        return err;
    hipStream_t st = (hipStream_t)stream;
    if (identity) {
        const dim3 grid((unsigned)((M + 31) / 32));
#define ALM_CALL(N) hipLaunchKernelGGL((fsq_decode_identity_kernel<N>), grid, dim3(256), 0, st, idx, ldi, consts, out, ldo, M, ncols)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
    } else {
        const dim3 grid((unsigned)((M + PQ_ROWS - 1) / PQ_ROWS));
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
    if (!pq_in_limits(dim_g, d, 1, FSQ_MAX_D)) return -1;
    const int ch = pq_chunk(M);
    const long long n = (long long)((M + ch - 1) / ch) * pq_epad(dim_g, d);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_fsq_bwd(const float* g, long long ldg, const float* x, long long ldx, const double* z, const float* W_in, const float* W_out,
                           const float* consts, float* dx, long long ldd, float* dW_in, float* db_in, float* dW_out, float* db_out, float* ws,
                           long long ws_floats, int M, int dim_g, int d, int Q, int k, void* stream) {
    bool identity, vec;
    if (const int err = pq_check(consts != nullptr, M, dim_g, d, Q, FSQ_MAX_D, 0, k, Q - 1, {{g, ldg}, {x, ldx}, {dx, ldd}}, {W_in, W_out},
                                 {W_in, W_out, ws}, identity, vec))
        return err;
    hipStream_t st = (hipStream_t)stream;
    if (identity) {
        const dim3 grid((unsigned)((M + 31) / 32));
#define ALM_CALL(N) hipLaunchKernelGGL((fsq_bwd_identity_kernel<N>), grid, dim3(256), 0, st, g, ldg, x, ldx, consts, dx, ldd, M, Q, k)
        ALM_FSQ_D(ALM_CALL)
#undef ALM_CALL
        ALM_LAUNCH_CHECK();
        return 0;
    }
    if (!z || !dW_in || !db_in || !dW_out || !db_out || !ws) return ALM_ERR_BAD_ARG;
    const int ch = pq_chunk(M), NC = (M + ch - 1) / ch;
    const long long epad = pq_epad(dim_g, d), need = (long long)NC * epad;
    if (need > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
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
