// Residual lookup-free quantization (LFQ, arXiv 2310.05737, in the residual form of vector-quantize-pytorch's GroupedResidualLFQ; restated in
// tests/lfq_restated.py) for gfx950: forward with the entropy / commitment losses, decode and backward, fp32 tensors, no float atomics (every output
// is one fixed-order chain, bitwise reproducible run to run).  Per group, d = log2(codebook_size), Q layers, k = last active layer, M tokens:
//
//     z = W_in x + b_in                                       W_in [d][dim_g]   (identity when dim_g == d: no weights at all)
//     r_0 = z ;  for q in 0..k, s_q = 2^-q:  bit_q[j] = r_q[j] > 0 ;  quant_q[j] = bit ? +s_q : -s_q ;  idx_q = sum_j bit_q[j] 2^(d-1-j)
//                                            r_{q+1} = r_q - quant_q
//     zsum = sum_q quant_q ;  out = W_out zsum + b_out        W_out [dim_g][d]
//     training:  p_m = softmax_c(2 tau <r_q[m], C_q[c]>),  C_q[c][j] = +-s_q by the bits of c,  H(t) = -sum_c t_c log max(t_c, eps)
//                loss_q = w_e (mean_m H(p_m) - gamma H(mean_m p_m)) + w_c mean_{m,j} (r_q - quant_q)^2
//
// Precision.  As in fsq.hip, z and the chain are carried in DOUBLE: the logit of layer q multiplies an error of z by 2 tau 2^-q (200 at layer 0), and
// the bits of the deep layers are signs of differences of nearly equal numbers.  The dot product of fp32 inputs is exact to 1e-16 in double and
// s_q = 2^-q is exact, so the indices are those of float64 arithmetic on the same fp32 inputs.  The saved z [M][d] is double.
//
// The softmax.  With a_j = 2 tau s_q r_q[j] the logit of code c is sum_j sigma_cj a_j, so the softmax factorises over the bits:
//     log P_j(+-) = +-a_j - |a_j| - log1p(exp(-2 |a_j|)),    p_c = prod_j P_j(sigma_cj),    log p_c = sum_j log P_j(sigma_cj)
// with no max pass and no overflow.  Because of the eps clamp the entropy is not the sum of d Bernoulli entropies: all 2^d probabilities are formed,
// each as ONE product of a low-half (<= 5 bits) and a high-half table entry, and its logarithm as one sum -- no exp / log per code.  All in double.
//
// Kernels.  The projections, the tiling and the backward's skeleton are csrc/proj_quant.hpp (LD = 16 lanes per row).  forward: (1) lfq_fwd_kernel:
// project_in, the chain with thread <-> (row, j), project_out; (2) lfq_stats_kernel, grid (row chunks, k + 1 layers): per tile of 16 rows the per-bit values and the two
// half tables in LDS, then thread <-> code (4 codes a thread at d = 10) runs over the rows and keeps sum_m p_mc and sum p log max(p, eps) in registers;
// the chunk's partials go to the caller's workspace; (3) lfq_finish_kernel, one workgroup per layer: adds the chunks in chunk order, writes
// avg [Q][2^d] and the loss.  backward: (1) lfq_bwd_loss_kernel, grid (M / 64, k + 1), thread <-> row: the row's low-half table in LDS ([entry][row],
// conflict-free), the high half formed per outer iteration, the d + 1 sums over the codes (u-bar and S_j) in registers; writes g_loss[q] dloss_q/dr_q
// [Q][M][d]; (2) lfq_bwd_kernel: proj_bwd with dz = (k + 1) g_z + the layers' loss gradients in layer order; (3) the chunk-order reduction of the
// parameter gradients.
#include "proj_quant.hpp"

namespace {

constexpr int LFQ_MAX_D = 10;
constexpr int LFQ_LD = 16;                                         // lanes (and LDS entries) per row in the chain phases: d <= 10 padded to 16
constexpr int LFQ_HALF = 5;                                        // bits of the low-half table
constexpr int LFQ_BROWS = 64;                                      // rows (= threads) of a workgroup of lfq_bwd_loss_kernel
constexpr double LFQ_EPS = 1e-5;

// The forward chain of dimension j of one row, called by ALL 16 lanes of a row (`active` = j < d and the row exists).  Returns zsum[j]; writes the
// row's indices (idx_row = idx + row * ldi, Q columns, -1 past k), lane q % 16 storing column q
__device__ __forceinline__ float chain_fwd(double res, bool active, int j, int d, int Q, int k, long long* __restrict__ idx_row) {
    const int weight = active ? 1 << (d - 1 - j) : 0;
    double zsum = 0.0, s = 1.0;                                    // s = 2^-q, exact
    for (int q = 0; q < Q; ++q) {
        int code = -1;
        if (q <= k) {                                              // workgroup-uniform
            const bool bit = res > 0.0;                            // 0 counts as not set
            code = bit ? weight : 0;
            code += __shfl_xor(code, 1, 64);
            code += __shfl_xor(code, 2, 64);
            code += __shfl_xor(code, 4, 64);
            code += __shfl_xor(code, 8, 64);
            const double quant = bit ? s : -s;
            zsum += quant;
            res -= quant;
            s *= 0.5;
        }
        if (idx_row && j == (q & 15)) idx_row[q] = (long long)code;
    }
    return (float)zsum;
}

// r_q[j] of one row from z[j]: q steps of the chain
__device__ __forceinline__ double chain_to(double res, int q) {
    double s = 1.0;
    for (int i = 0; i < q; ++i) {
        res -= res > 0.0 ? s : -s;
        s *= 0.5;
    }
    return res;
}

// zsum[j] of one row from z[j] (layers 0 .. k)
__device__ __forceinline__ float chain_zsum(double res, int k) {
    double s = 1.0, zs = 0.0;
    for (int q = 0; q <= k; ++q) {
        const double quant = res > 0.0 ? s : -s;
        zs += quant;
        res -= quant;
        s *= 0.5;
    }
    return (float)zs;
}

// zsum[j] of one row from its code indices (columns 0 .. ncols - 1 of idx_row; a negative entry contributes nothing)
__device__ __forceinline__ float codes_to_zsum(const long long* __restrict__ idx_row, int ncols, int j, int d) {
    float zs = 0.f, s = 1.f;
    for (int q = 0; q < ncols; ++q) {
        const long long id = idx_row[q];
        if (id >= 0) zs += (id >> (d - 1 - j)) & 1 ? s : -s;
        s *= 0.5f;
    }
    return zs;
}

// grid ceil(M / 16), 256 threads
template <int D, bool VEC>
__global__ __launch_bounds__(256) void lfq_fwd_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ W_in,
                                                      const float* __restrict__ b_in, const float* __restrict__ W_out, const float* __restrict__ b_out,
                                                      long long* __restrict__ idx, long long ldi, float* __restrict__ out, long long ldo,
                                                      double* __restrict__ z_out, int M, int dim_g, int Q, int k) {
    __shared__ double zl[PQ_ROWS * LFQ_LD];
    __shared__ float zs[PQ_ROWS * LFQ_LD];
    const long long row0 = (long long)blockIdx.x * PQ_ROWS;
    project_in<D, VEC, LFQ_LD>(x, ldx, W_in, b_in, zl, row0, M, dim_g);
    __syncthreads();
    {
        const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
        const long long row = row0 + r;
        const bool active = j < D && row < M;
        const double zv = zl[r * LFQ_LD + (j < D ? j : 0)];
        if (z_out && active) z_out[row * D + j] = zv;
        const float zsum = chain_fwd(zv, active, j, D, Q, k, row < M ? idx + row * ldi : nullptr);
        if (j < D) zs[r * LFQ_LD + j] = zsum;
    }
    __syncthreads();
    project_out<D, VEC, LFQ_LD>(zs, W_out, b_out, out, ldo, row0, M, dim_g);
}

// dim_g == d, no projections: thread <-> (row, j), 16 rows per workgroup
__global__ __launch_bounds__(256) void lfq_fwd_identity_kernel(const float* __restrict__ x, long long ldx, long long* __restrict__ idx, long long ldi,
                                                               float* __restrict__ out, long long ldo, double* __restrict__ z_out, int M, int d, int Q,
                                                               int k) {
    const int j = threadIdx.x & 15;
    const long long row = (long long)blockIdx.x * PQ_ROWS + (threadIdx.x >> 4);
    const bool active = j < d && row < M;
    const double zv = active ? (double)x[row * ldx + j] : 0.0;
    if (z_out && active) z_out[row * d + j] = zv;
    const float zsum = chain_fwd(zv, active, j, d, Q, k, row < M ? idx + row * ldi : nullptr);
    if (active) out[row * ldo + j] = zsum;
}

template <int D, bool VEC>
__global__ __launch_bounds__(256) void lfq_decode_kernel(const long long* __restrict__ idx, long long ldi, const float* __restrict__ W_out,
                                                         const float* __restrict__ b_out, float* __restrict__ out, long long ldo, int M, int dim_g,
                                                         int ncols) {
    __shared__ float zs[PQ_ROWS * LFQ_LD];
    const long long row0 = (long long)blockIdx.x * PQ_ROWS;
    {
        const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
        const long long row = row0 + r;
        if (j < D) zs[r * LFQ_LD + j] = row < M ? codes_to_zsum(idx + row * ldi, ncols, j, D) : 0.f;
    }
    __syncthreads();
    project_out<D, VEC, LFQ_LD>(zs, W_out, b_out, out, ldo, row0, M, dim_g);
}

__global__ __launch_bounds__(256) void lfq_decode_identity_kernel(const long long* __restrict__ idx, long long ldi, float* __restrict__ out,
                                                                  long long ldo, int M, int d, int ncols) {
    const int j = threadIdx.x & 15;
    const long long row = (long long)blockIdx.x * PQ_ROWS + (threadIdx.x >> 4);
    if (j < d && row < M) out[row * ldo + j] = codes_to_zsum(idx + row * ldi, ncols, j, d);
}

// log P(+), log P(-) of one bit with logit half-difference a: the two-entry softmax over (+a, -a)
__device__ __forceinline__ void bit_logprobs(double a, double& lp, double& lm) {
    const double aa = fabs(a), base = -aa - log1p(exp(-2.0 * aa));
    lp = a + base;
    lm = base - a;
}

// grid (NC row chunks of `chunk` rows, k + 1 layers), 256 threads.  ws: P [Q][NC][2^d] | Hs [Q][NC] | Cs [Q][NC] (doubles):
// P = sum over the chunk's rows of p_mc, Hs = sum_m sum_c p log max(p, eps) (= - sum_m H(p_m)), Cs = sum_{m,j} (r_q - quant_q)^2
__global__ __launch_bounds__(256) void lfq_stats_kernel(const double* __restrict__ z, double* __restrict__ ws, int M, int d, int Q, int chunk, int NC,
                                                        double tau2) {
    __shared__ double pb[PQ_ROWS][LFQ_MAX_D][2], lb[PQ_ROWS][LFQ_MAX_D][2];          // per bit: [.][j][1] = P(+), [.][j][0] = P(-)
    __shared__ double TP[PQ_ROWS][64], TL[PQ_ROWS][64];                                // per row: entries 0 .. 31 the low half, 32 .. 63 the high half
    __shared__ double red[4];
    const int q = blockIdx.y, tid = threadIdx.x;
    const int dl = d < LFQ_HALF ? d : LFQ_HALF, dh = d - dl, nl = 1 << dl, nh = 1 << dh, ncodes = 1 << d;
    const double s = ldexp(1.0, -q), log_eps = log(LFQ_EPS);
    const long long r_begin = (long long)blockIdx.x * chunk;
    const long long r_end = r_begin + chunk < M ? r_begin + chunk : M;
    double accp[4] = {0.0, 0.0, 0.0, 0.0}, hs = 0.0, cs = 0.0;
    for (long long row0 = r_begin; row0 < r_end; row0 += PQ_ROWS) {
        const int nrows = r_end - row0 < PQ_ROWS ? (int)(r_end - row0) : PQ_ROWS;
        {                                                          // (a) thread <-> (row, j): r_q[j], the bit's two probabilities, the commitment term
            const int r = tid >> 4, j = tid & 15;
            if (j < d && r < nrows) {
                const double res = chain_to(z[(row0 + r) * d + j], q);
                double lp, lm;
                bit_logprobs(tau2 * s * res, lp, lm);
                lb[r][j][1] = lp, lb[r][j][0] = lm;
                pb[r][j][1] = exp(lp), pb[r][j][0] = exp(lm);
                const double e = res - (res > 0.0 ? s : -s);
                cs += e * e;
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {                              // (b) the half tables: 16 rows x 64 entries, 4 a thread
            const int e = tid + 256 * t, r = e >> 6, ent = e & 63;
            if (r < nrows) {
                const bool low = ent < 32;
                const int code = low ? ent : ent - 32, nbits = low ? dl : dh, j0 = low ? d - 1 : dh - 1;      // bit b of the half <-> dimension j0 - b
                if (code < (low ? nl : nh)) {
                    double p = 1.0, l = 0.0;
                    for (int b = 0; b < nbits; ++b) {
                        const int sg = (code >> b) & 1;
                        p *= pb[r][j0 - b][sg];
                        l += lb[r][j0 - b][sg];
                    }
                    TP[r][ent] = p, TL[r][ent] = l;
                }
            }
        }
        __syncthreads();
        for (int r = 0; r < nrows; ++r) {                          // (c) thread <-> codes tid, tid + 256, ..
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = tid + 256 * i;
                if (c < ncodes) {
                    const double p = TP[r][32 + (c >> dl)] * TP[r][c & (nl - 1)];
                    const double lp = TL[r][32 + (c >> dl)] + TL[r][c & (nl - 1)];
                    hs += p * (p >= LFQ_EPS ? lp : log_eps);
                    accp[i] += p;
                }
            }
        }
        __syncthreads();
    }
    double* P = ws + ((long long)q * NC + blockIdx.x) * ncodes;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (tid + 256 * i < ncodes) P[tid + 256 * i] = accp[i];
    const double hsum = block_sum_d(hs, red), csum = block_sum_d(cs, red);
    if (tid == 0) {
        double* S = ws + (long long)Q * NC * ncodes;
        S[(long long)q * NC + blockIdx.x] = hsum;
        S[(long long)Q * NC + (long long)q * NC + blockIdx.x] = csum;
    }
}

// grid Q, 256 threads: the chunks in chunk order -> avg [Q][2^d], losses [Q]
__global__ __launch_bounds__(256) void lfq_finish_kernel(const double* __restrict__ ws, double* __restrict__ avg, float* __restrict__ losses, int M,
                                                         int d, int Q, int k, int NC, double w_e, double w_c, double gamma) {
    __shared__ double red[4];
    const int q = blockIdx.x, tid = threadIdx.x, ncodes = 1 << d;
    if (q > k) {                                                   // a layer quantize dropout left out: zero loss, zero row
        for (int c = tid; c < ncodes; c += 256) avg[(long long)q * ncodes + c] = 0.0;
        if (tid == 0) losses[q] = 0.f;
        return;
    }
    double h = 0.0;
    for (int c = tid; c < ncodes; c += 256) {
        const double* P = ws + (long long)q * NC * ncodes + c;
        double a = 0.0;
        for (int i = 0; i < NC; ++i) a += P[(long long)i * ncodes];
        a /= (double)M;
        avg[(long long)q * ncodes + c] = a;
        h -= a * log(a > LFQ_EPS ? a : LFQ_EPS);
    }
    const double h_avg = block_sum_d(h, red);
    if (tid == 0) {
        const double* S = ws + (long long)Q * NC * ncodes;
        double hsum = 0.0, csum = 0.0;
        for (int i = 0; i < NC; ++i) hsum += S[(long long)q * NC + i];
        for (int i = 0; i < NC; ++i) csum += S[(long long)Q * NC + (long long)q * NC + i];
        const double ent = -hsum / (double)M - gamma * h_avg;
        const double com = w_c > 0.0 ? w_c * csum / ((double)M * d) : 0.0;
        losses[q] = (float)(w_e * ent + com);
    }
}

// grid (ceil(M / 64), k + 1), 64 threads, thread <-> row.  gl [Q][M][d] = g_loss[q] * d loss_q / d r_q:
//     u_c = f'(p_c) - gamma f'(avg_c), f'(t) = -(log max(t, eps) + [t >= eps]);  u-bar = sum_c p_c u_c;  S_j = sum_c sigma_cj p_c u_c
//     d loss_q / d r_q[j] = (w_e / M) 2 tau s_q (S_j - u-bar tanh(a_j)) + w_c 2 (r_q - quant_q)[j] / (M d)
// Bit b of a code <-> dimension d - 1 - b; the per-bit registers are indexed by b.
__global__ __launch_bounds__(LFQ_BROWS) void lfq_bwd_loss_kernel(const double* __restrict__ z, const double* __restrict__ avg,
                                                                 const float* __restrict__ g_loss, float* __restrict__ gl, int M, int d, double tau2,
                                                                 double w_e, double w_c, double gamma) {
    __shared__ double B[1 << LFQ_MAX_D];                           // -gamma f'(avg_c)
    __shared__ double TP[1 << LFQ_HALF][LFQ_BROWS], TL[1 << LFQ_HALF][LFQ_BROWS];       // the row's low-half table, [entry][row]
    const int q = blockIdx.y, tid = threadIdx.x;
    const int dl = d < LFQ_HALF ? d : LFQ_HALF, dh = d - dl, nl = 1 << dl, nh = 1 << dh, ncodes = 1 << d;
    const double s = ldexp(1.0, -q), log_eps = log(LFQ_EPS);
    for (int c = tid; c < ncodes; c += LFQ_BROWS) {
        const double a = avg[(long long)q * ncodes + c];
        B[c] = gamma * (log(a > LFQ_EPS ? a : LFQ_EPS) + (a >= LFQ_EPS ? 1.0 : 0.0));
    }
    __syncthreads();
    const long long row = (long long)blockIdx.x * LFQ_BROWS + tid;
    if (row >= M) return;
    double Pp[LFQ_MAX_D], Pm[LFQ_MAX_D], Lp[LFQ_MAX_D], Lm[LFQ_MAX_D], err[LFQ_MAX_D], S[LFQ_MAX_D];
#pragma unroll
    for (int b = 0; b < LFQ_MAX_D; ++b) {
        Pp[b] = Pm[b] = 1.0, Lp[b] = Lm[b] = 0.0, err[b] = 0.0, S[b] = 0.0;
        if (b < d) {
            const double res = chain_to(z[row * d + (d - 1 - b)], q);
            bit_logprobs(tau2 * s * res, Lp[b], Lm[b]);
            Pp[b] = exp(Lp[b]), Pm[b] = exp(Lm[b]);
            err[b] = res - (res > 0.0 ? s : -s);
        }
    }
    for (int e = 0; e < nl; ++e) {
        double p = 1.0, l = 0.0;
#pragma unroll
        for (int b = 0; b < LFQ_HALF; ++b)
            if (b < dl) {
                const bool sg = (e >> b) & 1;
                p *= sg ? Pp[b] : Pm[b];
                l += sg ? Lp[b] : Lm[b];
            }
        TP[e][tid] = p, TL[e][tid] = l;
    }
    double ubar = 0.0;
    for (int ch = 0; ch < nh; ++ch) {
        double ph = 1.0, lh = 0.0;
#pragma unroll
        for (int b = 0; b < LFQ_HALF; ++b)
            if (b < dh) {
                const bool sg = (ch >> b) & 1;
                ph *= sg ? Pp[LFQ_HALF + b] : Pm[LFQ_HALF + b];
                lh += sg ? Lp[LFQ_HALF + b] : Lm[LFQ_HALF + b];
            }
        double A = 0.0;
        for (int cl = 0; cl < nl; ++cl) {
            const double p = ph * TP[cl][tid], lp = lh + TL[cl][tid];
            const bool big = p >= LFQ_EPS;
            const double u = B[(ch << dl) | cl] - ((big ? lp : log_eps) + (big ? 1.0 : 0.0));
            const double w = p * u;
            A += w;
#pragma unroll
            for (int b = 0; b < LFQ_HALF; ++b) S[b] += (cl >> b) & 1 ? w : -w;
        }
        ubar += A;
#pragma unroll
        for (int b = 0; b < LFQ_HALF; ++b) S[LFQ_HALF + b] += (ch >> b) & 1 ? A : -A;
    }
    const double gq = (double)g_loss[q], ce = gq * w_e / (double)M * tau2 * s, cc = w_c > 0.0 ? gq * w_c * 2.0 / ((double)M * d) : 0.0;
    float* o = gl + ((long long)q * M + row) * d;
#pragma unroll
    for (int b = 0; b < LFQ_MAX_D; ++b)
        if (b < d) o[d - 1 - b] = (float)(ce * (S[b] - ubar * (Pp[b] - Pm[b])) + cc * err[b]);
}

// grid = row chunks (`chunk` rows each, a multiple of 16), 256 threads; partials ws [chunk][epad]: dW_in [D][dim_g] | dW_out [dim_g][D] | db_out
// [dim_g] | db_in [D].  gl: the loss gradients [Q][M][D] of lfq_bwd_loss_kernel, or null
template <int D, bool VEC>
__global__ __launch_bounds__(256) void lfq_bwd_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ x, long long ldx,
                                                      const double* __restrict__ z, const float* __restrict__ gl, const float* __restrict__ W_in,
                                                      const float* __restrict__ W_out, float* __restrict__ dx, long long ldd, float* __restrict__ ws,
                                                      int M, int dim_g, int k, int chunk, long long epad) {
    proj_bwd<D, VEC, LFQ_LD>(g, ldg, x, ldx, W_in, W_out, dx, ldd, ws, M, dim_g, chunk, epad, [=](long long row, int j, float gzj, float& zsum) {
        float dz = (float)(k + 1) * gzj;
        if (gl)
            for (int q = 0; q <= k; ++q) dz += gl[((long long)q * M + row) * D + j];
        zsum = chain_zsum(z[row * D + j], k);
        return dz;
    });
}

__global__ __launch_bounds__(64) void lfq_bwd_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW_in, float* __restrict__ db_in,
                                                            float* __restrict__ dW_out, float* __restrict__ db_out, long long n_w, int dim_g, int d,
                                                            long long epad, int NC) {
    proj_bwd_reduce(ws, dW_in, db_in, dW_out, db_out, n_w, dim_g, d, epad, NC);
}

// dim_g == d: dx = (k + 1) g + the loss gradients, thread <-> (row, j)
__global__ __launch_bounds__(256) void lfq_bwd_identity_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ gl,
                                                               float* __restrict__ dx, long long ldd, int M, int d, int k) {
    const int j = threadIdx.x & 15;
    const long long row = (long long)blockIdx.x * PQ_ROWS + (threadIdx.x >> 4);
    if (j < d && row < M) {
        float v = (float)(k + 1) * g[row * ldg + j];
        if (gl)
            for (int q = 0; q <= k; ++q) v += gl[((long long)q * M + row) * d + j];
        dx[row * ldd + j] = v;
    }
}

// rows of a chunk of the forward's code-distribution partials: 64, doubled until there are at most 256 chunks
inline int lfq_stats_chunk(int M) { return row_chunk(M, 64, 256); }

#define ALM_LFQ_D(CALL) ALM_PQ_D(LFQ_MAX_D, CALL)

}  // namespace

// doubles of the caller-owned workspace of a training-mode alm_lfq_fwd: row chunks (64 rows, doubled until there are at most 256 chunks) x Q layers
// x (2^d + 2); -1 outside the limits or past 2^31
extern "C" int alm_lfq_fwd_ws_doubles(int M, int d, int Q) {
    if (M <= 0 || d <= 0 || Q <= 0 || !pq_in_limits(1, d, Q, LFQ_MAX_D)) return -1;
    const int ch = lfq_stats_chunk(M);
    const long long n = (long long)((M + ch - 1) / ch) * Q * ((1LL << d) + 2);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_lfq_fwd(const float* x, long long ldx, const float* W_in, const float* b_in, const float* W_out, const float* b_out, long long* idx,
                           long long ldi, float* out, long long ldo, double* z, float* losses, double* avg, double* ws, long long ws_doubles, int M,
                           int dim_g, int d, int Q, int k, float inv_temperature, float entropy_w, float commit_w, float gamma, void* stream) {
    bool identity, vec;
    if (const int err = pq_check(idx && ldi >= Q, M, dim_g, d, Q, LFQ_MAX_D, 0, k, Q - 1, {{x, ldx}, {out, ldo}}, {W_in, b_in, W_out, b_out},
                                 {W_in, W_out, b_out}, identity, vec))
        return err;
    const int sch = lfq_stats_chunk(M), SNC = (M + sch - 1) / sch;
    if (losses) {
        if (!z || !avg || !ws || !(inv_temperature > 0.f)) return ALM_ERR_BAD_ARG;
        const long long need = (long long)SNC * Q * ((1LL << d) + 2);
        if (need > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
        if (ws_doubles < need) return ALM_ERR_BAD_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((M + PQ_ROWS - 1) / PQ_ROWS));
    if (identity) {
        hipLaunchKernelGGL(lfq_fwd_identity_kernel, grid, dim3(256), 0, st, x, ldx, idx, ldi, out, ldo, z, M, d, Q, k);
    } else {
#define ALM_CALL(N)                                                                                                                                 \
    if (vec) hipLaunchKernelGGL((lfq_fwd_kernel<N, true>), grid, dim3(256), 0, st, x, ldx, W_in, b_in, W_out, b_out, idx, ldi, out, ldo, z, M,     \
                                dim_g, Q, k);                                                                                                       \
    else hipLaunchKernelGGL((lfq_fwd_kernel<N, false>), grid, dim3(256), 0, st, x, ldx, W_in, b_in, W_out, b_out, idx, ldi, out, ldo, z, M, dim_g, \
                            Q, k)
        ALM_LFQ_D(ALM_CALL)
#undef ALM_CALL
    }
    ALM_LAUNCH_CHECK();
    if (losses) {
        hipLaunchKernelGGL(lfq_stats_kernel, dim3((unsigned)SNC, (unsigned)(k + 1)), dim3(256), 0, st, z, ws, M, d, Q, sch, SNC,
                           2.0 * (double)inv_temperature);
        ALM_LAUNCH_CHECK();
        hipLaunchKernelGGL(lfq_finish_kernel, dim3((unsigned)Q), dim3(256), 0, st, ws, avg, losses, M, d, Q, k, SNC, (double)entropy_w, (double)commit_w,
                           (double)gamma);
        ALM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int alm_lfq_decode(const long long* idx, long long ldi, const float* W_out, const float* b_out, float* out, long long ldo, int M, int dim_g,
                              int d, int Q, int ncols, void* stream) {
    bool identity, vec;
    if (const int err = pq_check(idx && ldi >= ncols, M, dim_g, d, Q, LFQ_MAX_D, 1, ncols, Q, {{out, ldo}}, {W_out, b_out}, {W_out, b_out}, identity, vec))
        return err;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((M + PQ_ROWS - 1) / PQ_ROWS));
    if (identity) {
        hipLaunchKernelGGL(lfq_decode_identity_kernel, grid, dim3(256), 0, st, idx, ldi, out, ldo, M, d, ncols);
    } else {
#define ALM_CALL(N)                                                                                                             \
    if (vec) hipLaunchKernelGGL((lfq_decode_kernel<N, true>), grid, dim3(256), 0, st, idx, ldi, W_out, b_out, out, ldo, M, dim_g, ncols); \
    else hipLaunchKernelGGL((lfq_decode_kernel<N, false>), grid, dim3(256), 0, st, idx, ldi, W_out, b_out, out, ldo, M, dim_g, ncols)
        ALM_LFQ_D(ALM_CALL)
#undef ALM_CALL
    }
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of alm_lfq_bwd: the per-layer loss gradients Q x M x d (rounded up to 4), then row chunks (32 rows, doubled
// until there are at most 1024 chunks) x the parameter gradients' 2 d dim_g + dim_g + d floats rounded up to 4 (none in the identity case
// dim_g == d); -1 outside the limits or past 2^31
extern "C" int alm_lfq_bwd_ws_floats(int M, int dim_g, int d, int Q) {
    if (M <= 0 || dim_g <= 0 || d <= 0 || Q <= 0 || !pq_in_limits(dim_g, d, Q, LFQ_MAX_D)) return -1;
    long long n = up4((long long)Q * M * d);
    if (dim_g != d) {
        const int ch = pq_chunk(M);
        n += (long long)((M + ch - 1) / ch) * pq_epad(dim_g, d);
    }
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_lfq_bwd(const float* g, long long ldg, const float* g_loss, const float* x, long long ldx, const double* z, const double* avg,
                           const float* W_in, const float* W_out, float* dx, long long ldd, float* dW_in, float* db_in, float* dW_out, float* db_out,
                           float* ws, long long ws_floats, int M, int dim_g, int d, int Q, int k, float inv_temperature, float entropy_w, float commit_w,
                           float gamma, void* stream) {
    bool identity, vec;                                            // ws stands for the partials: they start a multiple of 16 bytes behind it
    if (const int err = pq_check(z && ws, M, dim_g, d, Q, LFQ_MAX_D, 0, k, Q - 1, {{g, ldg}, {x, ldx}, {dx, ldd}}, {W_in, W_out}, {W_in, W_out, ws},
                                 identity, vec))
        return err;
    if (g_loss && (!avg || !(inv_temperature > 0.f))) return ALM_ERR_BAD_ARG;
    if (!identity && (!dW_in || !db_in || !dW_out || !db_out)) return ALM_ERR_BAD_ARG;
    const int ch = pq_chunk(M), NC = (M + ch - 1) / ch;
    const long long n_gl = up4((long long)Q * M * d), epad = pq_epad(dim_g, d), need = n_gl + (identity ? 0 : (long long)NC * epad);
    if (need > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* gl = g_loss ? ws : nullptr;
    float* part = ws + n_gl;
    if (g_loss) {
        hipLaunchKernelGGL(lfq_bwd_loss_kernel, dim3((unsigned)((M + LFQ_BROWS - 1) / LFQ_BROWS), (unsigned)(k + 1)), dim3(LFQ_BROWS), 0, st, z, avg,
                           g_loss, gl, M, d, 2.0 * (double)inv_temperature, (double)entropy_w, (double)commit_w, (double)gamma);
        ALM_LAUNCH_CHECK();
    }
    if (identity) {
        hipLaunchKernelGGL(lfq_bwd_identity_kernel, dim3((unsigned)((M + PQ_ROWS - 1) / PQ_ROWS)), dim3(256), 0, st, g, ldg, gl, dx, ldd, M, d, k);
        ALM_LAUNCH_CHECK();
        return 0;
    }
#define ALM_CALL(N)                                                                                                                               \
    if (vec) hipLaunchKernelGGL((lfq_bwd_kernel<N, true>), dim3((unsigned)NC), dim3(256), 0, st, g, ldg, x, ldx, z, gl, W_in, W_out, dx, ldd,    \
                                part, M, dim_g, k, ch, epad);                                                                                     \
    else hipLaunchKernelGGL((lfq_bwd_kernel<N, false>), dim3((unsigned)NC), dim3(256), 0, st, g, ldg, x, ldx, z, gl, W_in, W_out, dx, ldd, part, \
                            M, dim_g, k, ch, epad)
    ALM_LFQ_D(ALM_CALL)
#undef ALM_CALL
    ALM_LAUNCH_CHECK();
    const long long E = 2LL * d * dim_g + dim_g + d;
    hipLaunchKernelGGL(lfq_bwd_reduce_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, st, part, dW_in, db_in, dW_out, db_out, (long long)d * dim_g,
                       dim_g, d, epad, NC);
    ALM_LAUNCH_CHECK();
    return 0;
}
