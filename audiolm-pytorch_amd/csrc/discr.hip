// Wave discriminators of SoundStream training (reference soundstream.py:92-140 MultiScaleDiscriminator, :61-65 hinge losses, :634 AvgPool1d), fp32.
//
// Grouped strided zero-padded conv1d  y = act(conv1d(x, w, b, stride, padding, groups)),  act in {identity, LeakyReLU(0.1)}: forward, input
// gradient, weight + bias gradient.  The weights are read in nn.Conv1d's own layout [Cout][Cin / groups][k]: no derived image exists.  These layers
// are 4 input channels per group against 41 taps at stride 4 (or dense with 3 / 5 / 15 taps): latency- and LDS-bound, nothing for the MFMA pipe.
//   forward : one block = (batch, group, tile of 4 J output channels, 64 output steps); the input window of the reduce-channel chunk sits in LDS split
//             by stride phase (lane t reads phase-row element t + k / s: consecutive lanes, consecutive banks), the weights of the tile beside it
//             (wave-uniform reads: a broadcast).  wave w of the block owns output channels w J .. w J + J - 1.
//   dgrad   : the same tiling over (batch, group, tile of 4 J input channels, 64 input steps): a gather over the taps k = (u + p) mod s, + s, ... of
//             the window of g act'(y) staged in LDS -- no scatter, no atomics.
//   wgrad   : one block = (group, tile of output x input channels, split of the (batch, 64-step chunk) list); each thread keeps up to 12 of the tile's
//             Cout_t x Cin_t x k sums in registers over ALL chunks of its split (walked in list order), writes them to the split's slab of the workspace,
//             and discr_wgrad_reduce_kernel adds the slabs in split order.  The split count depends on the shapes only: gradients are bitwise reproducible.
// The activation's derivative comes from the saved OUTPUT (y > 0 <=> pre-activation > 0), like the ELU path of codec_bwd.hip.
//   masked  : the forward tiling with another epilogue, out = m(y) conv(v, w) without a bias, m(y) = 1 where the saved output y > 0 and 0.1 elsewhere
//             (y null: m = 1).  It is the derivative of dgrad with respect to its incoming gradient: the double backward of the gradient penalty.
//
// AvgPool1d(2 f, stride f, padding f), count_include_pad: y[t] = sum_{i < 2f} x[t f - f + i] / (2 f); its adjoint gathers the <= 2 windows over u.
// Loss reductions (hinge discriminator / hinge generator / L1 / squared error / complex L1 = mean modulus means): per-block partial sums over a contiguous span in a fixed lane
// order, then one block adds the partials in index order; the backward is elementwise and takes the upstream gradient from device memory.
// Gradient penalty (soundstream.py:70-83) weight / R sum_r (|G_r| - center)^2 of G [R][n]: the rows' sums of squares the same way (per-block spans of a
// row, partials added in index order), the R norms kept for the elementwise backward.
#include "common.hpp"

namespace {

constexpr int TT = 64;                   // steps per tile (one wave's lanes)
constexpr int XS_MAX = 6144;             // floats of the staged signal window
constexpr int WS_MAX = 4096;             // floats of the staged weights
constexpr int WG_ACC = 12;               // sums per thread of the weight gradient
constexpr float LEAK = 0.1f;
constexpr int ACT_MASKED = 2;            // forward epilogue of the masked form: no bias, times m(y)

struct GConvArgs {
    const float* x;      // forward: input [B][Cin][Tin]; dgrad: unused; wgrad: input
    const float* w;      // [Cout][cig][K]
    const float* bias;   // [Cout] (forward)
    const float* g;      // dL/dy [B][Cout][Tout] (backward)
    const float* y;      // saved output (backward, act; masked forward) or null
    float* out;          // forward: y; dgrad: dx; wgrad: workspace
    int B, Cin, Cout, Tin, Tout, K, s, p, G, cig, cog, act;      // forward act: 0 identity, 1 LeakyReLU, ACT_MASKED
    int chunk;           // reduce channels staged per round (forward: input, dgrad: output channels)
    int row;             // floats per staged signal row
    int tiles;           // channel tiles per group (forward: of cog, dgrad: of cig)
    int cot, cit, ncot, ncit, per, nchunk, nT;        // wgrad tiling
};

__device__ __forceinline__ int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <int J>
__global__ __launch_bounds__(256) void gconv_fwd_kernel(GConvArgs a) {
    __shared__ float xs[XS_MAX];
    __shared__ float ws[WS_MAX];
    const int tid = threadIdx.x, tl = tid & 63, cl = tid >> 6;
    constexpr int CT = 4 * J;
    const int t0 = blockIdx.x * TT, grp = blockIdx.y / a.tiles, co0 = (blockIdx.y % a.tiles) * CT, b = blockIdx.z;
    const int W = (TT - 1) * a.s + a.K, QW = a.row / a.s, pos0 = t0 * a.s - a.p;
    float acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0.f;
    for (int ci0 = 0; ci0 < a.cig; ci0 += a.chunk) {
        const int nci = min(a.chunk, a.cig - ci0);
        __syncthreads();
        for (int i = tid; i < nci * W; i += 256) {
            const int c = i / W, q = i - c * W, pos = pos0 + q;
            float v = 0.f;
            if (pos >= 0 && pos < a.Tin) v = a.x[((size_t)b * a.Cin + grp * a.cig + ci0 + c) * a.Tin + pos];
            xs[c * a.row + (q % a.s) * QW + q / a.s] = v;
        }
        const int nk = nci * a.K;
        for (int i = tid; i < CT * nk; i += 256) {
            const int co = i / nk, r = i - co * nk;
            float v = 0.f;
            if (co0 + co < a.cog) v = a.w[((size_t)(grp * a.cog + co0 + co) * a.cig + ci0) * a.K + r];
            ws[co * a.chunk * a.K + r] = v;
        }
        __syncthreads();
        for (int c = 0; c < nci; ++c) {
            const float* xr = xs + c * a.row + tl;
            const float* wr = ws + (cl * J * a.chunk + c) * a.K;
            int kq = 0, kr = 0;
            for (int k = 0; k < a.K; ++k) {
                const float xv = xr[kr * QW + kq];
#pragma unroll
                for (int j = 0; j < J; ++j) acc[j] = fmaf(wr[j * a.chunk * a.K + k], xv, acc[j]);
                if (++kr == a.s) { kr = 0; ++kq; }
            }
        }
    }
    const int t = t0 + tl;
    if (t < a.Tout) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int co = co0 + cl * J + j;
            if (co < a.cog) {
                const int cg = grp * a.cog + co;
                const size_t o = ((size_t)b * a.Cout + cg) * a.Tout + t;
                float v;
                if (a.act == ACT_MASKED) {
                    v = acc[j];
                    if (a.y && !(a.y[o] > 0.f)) v *= LEAK;
                } else {
                    v = acc[j] + a.bias[cg];
                    if (a.act) v = v > 0.f ? v : LEAK * v;
                }
                a.out[o] = v;
            }
        }
    }
}

template <int J>
__global__ __launch_bounds__(256) void gconv_dgrad_kernel(GConvArgs a) {
    __shared__ float gs[XS_MAX];
    __shared__ float ws[WS_MAX];
    const int tid = threadIdx.x, ul = tid & 63, cl = tid >> 6;
    constexpr int CT = 4 * J;
    const int u0 = blockIdx.x * TT, grp = blockIdx.y / a.tiles, ci0 = (blockIdx.y % a.tiles) * CT, b = blockIdx.z;
    const int tlo = floordiv(u0 + a.p - (a.K - 1), a.s), thi = floordiv(u0 + TT - 1 + a.p, a.s), GW = thi - tlo + 1;   // GW <= a.row
    const int u = u0 + ul, r = (u + a.p) % a.s, tt0 = (u + a.p - r) / a.s - tlo;
    float acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0.f;
    for (int co0 = 0; co0 < a.cog; co0 += a.chunk) {
        const int nco = min(a.chunk, a.cog - co0);
        __syncthreads();
        for (int i = tid; i < nco * GW; i += 256) {
            const int c = i / GW, q = i - c * GW, t = tlo + q;
            float v = 0.f;
            if (t >= 0 && t < a.Tout) {
                const size_t o = ((size_t)b * a.Cout + grp * a.cog + co0 + c) * a.Tout + t;
                v = a.g[o];
                if (a.act && !(a.y[o] > 0.f)) v *= LEAK;
            }
            gs[c * a.row + q] = v;
        }
        const int nk = CT * a.K;
        for (int i = tid; i < nco * nk; i += 256) {
            const int c = i / nk, rr = i - c * nk, ci = rr / a.K, k = rr - ci * a.K;
            float v = 0.f;
            if (ci0 + ci < a.cig) v = a.w[((size_t)(grp * a.cog + co0 + c) * a.cig + ci0 + ci) * a.K + k];
            ws[i] = v;                                          // [c][ci][k]
        }
        __syncthreads();
        for (int c = 0; c < nco; ++c) {
            const float* gr = gs + c * a.row;
            const float* wr = ws + (c * CT + cl * J) * a.K;
            int tt = tt0;
            for (int k = r; k < a.K; k += a.s, --tt) {
                const float gv = gr[tt];
#pragma unroll
                for (int j = 0; j < J; ++j) acc[j] = fmaf(wr[j * a.K + k], gv, acc[j]);
            }
        }
    }
    if (u < a.Tin) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int ci = ci0 + cl * J + j;
            if (ci < a.cig) a.out[((size_t)b * a.Cin + grp * a.cig + ci) * a.Tin + u] = acc[j];
        }
    }
}

// grid (splits, G * ncot * ncit); workspace slab of split sp: [numel(dw) + Cout] floats
template <int NJ>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(GConvArgs a) {
    __shared__ float xs[XS_MAX];
    __shared__ float gs[16 * (TT + 1)];
    const int tid = threadIdx.x, sp = blockIdx.x;
    int tile = blockIdx.y;
    const int cit_i = tile % a.ncit;
    tile /= a.ncit;
    const int cot_i = tile % a.ncot, grp = tile / a.ncot;
    const int co0 = cot_i * a.cot, ci0 = cit_i * a.cit;
    const int W = (TT - 1) * a.s + a.K, nout = a.cot * a.cit * a.K;
    float acc[NJ], bacc = 0.f;
    int goff[NJ], xoff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        acc[j] = 0.f;
        const int o = min(tid + j * 256, nout - 1);             // lanes past the tile recompute its last sum and do not store it
        const int co = o / (a.cit * a.K), rr = o - co * a.cit * a.K, ci = rr / a.K, k = rr - ci * a.K;
        goff[j] = co * (TT + 1);
        xoff[j] = ci * a.row + k;
    }
    const int c_lo = sp * a.per, c_hi = min(a.nchunk, c_lo + a.per);
    for (int ch = c_lo; ch < c_hi; ++ch) {
        const int b = ch / a.nT, t0 = (ch - b * a.nT) * TT, pos0 = t0 * a.s - a.p;
        __syncthreads();
        for (int i = tid; i < a.cit * W; i += 256) {
            const int c = i / W, q = i - c * W, pos = pos0 + q;
            float v = 0.f;
            if (ci0 + c < a.cig && pos >= 0 && pos < a.Tin) v = a.x[((size_t)b * a.Cin + grp * a.cig + ci0 + c) * a.Tin + pos];
            xs[c * a.row + q] = v;
        }
        for (int i = tid; i < a.cot * TT; i += 256) {
            const int c = i / TT, q = i - c * TT, t = t0 + q;
            float v = 0.f;
            if (co0 + c < a.cog && t < a.Tout) {
                const size_t o = ((size_t)b * a.Cout + grp * a.cog + co0 + c) * a.Tout + t;
                v = a.g[o];
                if (a.act && !(a.y[o] > 0.f)) v *= LEAK;
            }
            gs[c * (TT + 1) + q] = v;
        }
        __syncthreads();
        for (int t = 0; t < TT; ++t) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = fmaf(gs[goff[j] + t], xs[xoff[j] + t * a.s], acc[j]);
        }
        if (cit_i == 0 && tid < a.cot) {
            for (int t = 0; t < TT; ++t) bacc += gs[tid * (TT + 1) + t];
        }
    }
    const size_t ndw = (size_t)a.Cout * a.cig * a.K;
    float* slab = a.out + (size_t)sp * (ndw + a.Cout);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int o = tid + j * 256;
        if (o < nout) {
            const int co = o / (a.cit * a.K), rr = o - co * a.cit * a.K, ci = rr / a.K, k = rr - ci * a.K;
            if (co0 + co < a.cog && ci0 + ci < a.cig) slab[((size_t)(grp * a.cog + co0 + co) * a.cig + ci0 + ci) * a.K + k] = acc[j];
        }
    }
    if (cit_i == 0 && tid < a.cot && co0 + tid < a.cog) slab[ndw + grp * a.cog + co0 + tid] = bacc;
}

__global__ __launch_bounds__(256) void discr_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, long long ndw,
                                                                 int Cout, int splits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, n = ndw + Cout;
    if (i >= n) return;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += ws[(size_t)sp * n + i];
    if (i < ndw) dw[i] = s;
    else db[i - ndw] = s;
}

struct WgPlan { int cot, cit, ncot, ncit, nT, nchunk, per, splits, row; };

bool wgrad_plan(int B, int Cin, int Cout, int Tout, int K, int s, int G, WgPlan& p) {
    const int cig = Cin / G, cog = Cout / G;
    p.cot = min(cog, 16);
    p.cit = min(cig, 16);
    while (p.cot * p.cit * K > WG_ACC * 256 && (p.cot > 1 || p.cit > 1)) {
        if (p.cot >= p.cit) p.cot = (p.cot + 1) / 2;
        else p.cit = (p.cit + 1) / 2;
    }
    p.row = (TT - 1) * s + K;
    while (p.cit > 1 && (long long)p.cit * p.row > XS_MAX) p.cit = (p.cit + 1) / 2;
    if ((long long)p.cot * p.cit * K > WG_ACC * 256 || (long long)p.cit * p.row > XS_MAX) return false;
    p.ncot = (cog + p.cot - 1) / p.cot;
    p.ncit = (cig + p.cit - 1) / p.cit;
    p.nT = (Tout + TT - 1) / TT;
    const long long nchunk = (long long)B * p.nT, tiles = (long long)G * p.ncot * p.ncit;
    if (nchunk >= 0x7fffffffLL || tiles > 65535) return false;
    p.nchunk = (int)nchunk;
    long long want = (2048 + tiles - 1) / tiles;                     // ~2048 blocks in flight; a function of the shapes only
    if (want > nchunk) want = nchunk;
    if (want > 512) want = 512;
    p.per = (int)((nchunk + want - 1) / want);
    p.splits = (p.nchunk + p.per - 1) / p.per;
    return true;
}

bool conv_shape_ok(int B, int Cin, int Cout, int Tin, int K, int s, int p, int G) {
    return B > 0 && Cin > 0 && Cout > 0 && Tin > 0 && K > 0 && s > 0 && p >= 0 && G > 0 && Cin % G == 0 && Cout % G == 0 && (long long)Tin + 2LL * p >= K;
}

// ------------------------------------------------------------------------------------------------ pooling

__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long rows, int T, int Tout, int f) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * Tout) return;
    const long long r = i / Tout;
    const int t = (int)(i - r * Tout);
    const float* xr = x + r * T;
    float s = 0.f;
    for (int k = 0; k < 2 * f; ++k) {
        const long long pos = (long long)t * f - f + k;
        if (pos >= 0 && pos < T) s += xr[pos];
    }
    y[i] = s / (float)(2 * f);
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, long long rows, int T, int Tout, int f) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * T) return;
    const long long r = i / T;
    const int u = (int)(i - r * T), t = u / f;
    const float* gr = g + r * Tout;
    float s = gr[t];                                                 // t = u / f <= (T - 1) / f < Tout
    if (t + 1 < Tout) s += gr[t + 1];
    dx[i] = s / (float)(2 * f);
}

// ------------------------------------------------------------------------------------------------ loss reductions

constexpr int RED_SPAN = 4096, RED_MAX_BLOCKS = 1024;

__device__ __forceinline__ float loss_term(int mode, float a, float b) {
    switch (mode) {
        case ALM_LOSS_HINGE_DISCR: return fmaxf(1.f + a, 0.f) + fmaxf(1.f - b, 0.f);
        case ALM_LOSS_HINGE_GEN: return -a;
        case ALM_LOSS_L1: return fabsf(a - b);
        default: return (a - b) * (a - b);
    }
}

__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ part, long long n,
                                                           long long span, int mode) {
    const long long lo = (long long)blockIdx.x * span, hi = min(n, lo + span);
    float s = 0.f;
    if (mode == ALM_LOSS_L1_COMPLEX) {                              // n complex elements: the modulus of the difference of the (re, im) pairs
        for (long long i = lo + threadIdx.x; i < hi; i += 256) s += hypotf(a[2 * i] - b[2 * i], a[2 * i + 1] - b[2 * i + 1]);
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += 256) s += loss_term(mode, a[i], b ? b[i] : 0.f);
    }
    s = block_sum(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts, float scale) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[0] = s * scale;
}

__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gout,
                                                       float* __restrict__ da, float* __restrict__ db, long long n, float scale, int mode) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float g = gout[0] * scale;
    if (mode == ALM_LOSS_L1_COMPLEX) {                              // (a - b) / |a - b| g, 0 where a == b
        const float dr = a[2 * i] - b[2 * i], di = a[2 * i + 1] - b[2 * i + 1], r = hypotf(dr, di);
        const float gr = r > 0.f ? g * (dr / r) : 0.f, gi = r > 0.f ? g * (di / r) : 0.f;
        if (da) da[2 * i] = gr, da[2 * i + 1] = gi;
        if (db) db[2 * i] = -gr, db[2 * i + 1] = -gi;
        return;
    }
    float ga = 0.f, gb = 0.f;
    if (mode == ALM_LOSS_HINGE_DISCR) {
        ga = 1.f + a[i] > 0.f ? g : 0.f;
        gb = 1.f - b[i] > 0.f ? -g : 0.f;
    } else if (mode == ALM_LOSS_HINGE_GEN) {
        ga = -g;
    } else if (mode == ALM_LOSS_L1) {
        const float d = a[i] - b[i];
        ga = d > 0.f ? g : (d < 0.f ? -g : 0.f);
        gb = -ga;
    } else {
        ga = 2.f * g * (a[i] - b[i]);
        gb = -ga;
    }
    if (da) da[i] = ga;
    if (db) db[i] = gb;
}

// ------------------------------------------------------------------------------------------------ gradient penalty

// grid (nparts, R): this block's span of row r, squares summed in a fixed lane order, into part[r][blockIdx.x]
__global__ __launch_bounds__(256) void penalty_partial_kernel(const float* __restrict__ G, float* __restrict__ part, long long n, long long span) {
    const long long lo = (long long)blockIdx.x * span, hi = min(n, lo + span);
    const float* row = G + (size_t)blockIdx.y * n;
    float s = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) s = fmaf(row[i], row[i], s);
    s = block_sum(s);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// one block: the rows in order, each row's partials in index order; norms[r] = |G_r|, out = scale * sum_r (|G_r| - center)^2
__global__ __launch_bounds__(256) void penalty_final_kernel(const float* __restrict__ part, float* __restrict__ norms, float* __restrict__ out, int R,
                                                            int nparts, float scale, float center) {
    float total = 0.f;
    for (int r = 0; r < R; ++r) {
        float s = 0.f;
        for (int i = threadIdx.x; i < nparts; i += 256) s += part[(size_t)r * nparts + i];
        s = block_sum(s);
        const float nr = sqrtf(s), d = nr - center;
        total = fmaf(d, d, total);
        if (threadIdx.x == 0) norms[r] = nr;
    }
    if (threadIdx.x == 0) out[0] = total * scale;
}

// dG[r][i] = gout * scale * 2 (|G_r| - center) * G[r][i] / |G_r|, 0 for a row of norm 0
__global__ __launch_bounds__(256) void penalty_bwd_kernel(const float* __restrict__ G, const float* __restrict__ norms, const float* __restrict__ gout,
                                                          float* __restrict__ dG, long long n, float scale, float center) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float nr = norms[blockIdx.y];
    const size_t o = (size_t)blockIdx.y * n + i;
    dG[o] = nr > 0.f ? gout[0] * scale * 2.f * (nr - center) * (G[o] / nr) : 0.f;
}

constexpr int PEN_MAX_ROWS = 65535;

// span of a row per block and the blocks per row of the penalty's first stage
int penalty_parts(long long n, long long& span) {
    span = RED_SPAN;
    while ((n + span - 1) / span > RED_MAX_BLOCKS) span *= 2;
    return (int)((n + span - 1) / span);
}

int gconv_fwd_launch(GConvArgs& a, hipStream_t stream) {
    a.Tout = alm_gconv1d_out_len(a.Tin, a.K, a.s, a.p);
    a.cig = a.Cin / a.G, a.cog = a.Cout / a.G;
    const int J = a.cog > 4 ? 4 : 1, CT = 4 * J;
    const long long W = (long long)(TT - 1) * a.s + a.K;
    const long long row = (W + a.s - 1) / a.s * a.s;
    if (row > XS_MAX || (long long)CT * a.K > WS_MAX || (long long)a.Tin * a.s >= 0x3fffffffLL) return ALM_ERR_UNSUPPORTED;
    a.row = (int)row;
    a.chunk = (int)min((long long)a.cig, min(XS_MAX / row, (long long)WS_MAX / (CT * a.K)));
    a.tiles = (a.cog + CT - 1) / CT;
    const long long gy = (long long)a.G * a.tiles;
    if (gy > 65535 || a.B > 65535) return ALM_ERR_UNSUPPORTED;
    const dim3 grid((a.Tout + TT - 1) / TT, (unsigned)gy, a.B);
    if (J == 4) hipLaunchKernelGGL(gconv_fwd_kernel<4>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(gconv_fwd_kernel<1>, grid, dim3(256), 0, stream, a);
    ALM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int alm_gconv1d_out_len(int Tin, int ksize, int stride, int padding) {
    if (Tin <= 0 || ksize <= 0 || stride <= 0 || padding < 0 || (long long)Tin + 2LL * padding < ksize) return -1;
    return (int)(((long long)Tin + 2LL * padding - ksize) / stride + 1);
}

extern "C" int alm_gconv1d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int Tin, int ksize, int stride,
                               int padding, int groups, int act, void* stream) {
    if (!conv_shape_ok(B, Cin, Cout, Tin, ksize, stride, padding, groups) || (act != 0 && act != 1)) return ALM_ERR_BAD_ARG;
    GConvArgs a = {};
    a.x = x, a.w = w, a.bias = bias, a.out = y;
    a.B = B, a.Cin = Cin, a.Cout = Cout, a.Tin = Tin, a.K = ksize, a.s = stride, a.p = padding, a.G = groups, a.act = act;
    return gconv_fwd_launch(a, (hipStream_t)stream);
}

// out = m(y) conv1d(v, w) without a bias: the derivative of alm_gconv1d_dgrad(g, y, w) with respect to g, applied to v.  y null: no mask.
extern "C" int alm_gconv1d_fwd_masked(const float* v, const float* w, const float* y, float* out, int B, int Cin, int Cout, int Tin, int ksize, int stride,
                                      int padding, int groups, void* stream) {
    if (v == nullptr || w == nullptr || out == nullptr || !conv_shape_ok(B, Cin, Cout, Tin, ksize, stride, padding, groups)) return ALM_ERR_BAD_ARG;
    GConvArgs a = {};
    a.x = v, a.w = w, a.y = y, a.out = out;
    a.B = B, a.Cin = Cin, a.Cout = Cout, a.Tin = Tin, a.K = ksize, a.s = stride, a.p = padding, a.G = groups, a.act = ACT_MASKED;
    return gconv_fwd_launch(a, (hipStream_t)stream);
}

extern "C" int alm_gconv1d_dgrad(const float* g, const float* y, const float* w, float* dx, int B, int Cin, int Cout, int Tin, int ksize, int stride,
                                 int padding, int groups, void* stream) {
    if (!conv_shape_ok(B, Cin, Cout, Tin, ksize, stride, padding, groups)) return ALM_ERR_BAD_ARG;
    GConvArgs a = {};
    a.g = g, a.y = y, a.w = w, a.out = dx;
    a.B = B, a.Cin = Cin, a.Cout = Cout, a.Tin = Tin, a.K = ksize, a.s = stride, a.p = padding, a.G = groups, a.act = y != nullptr;
    a.Tout = alm_gconv1d_out_len(Tin, ksize, stride, padding);
    a.cig = Cin / groups, a.cog = Cout / groups;
    const int J = a.cig > 4 ? 4 : 1, CT = 4 * J;
    const long long row = (long long)(TT + ksize - 2) / stride + 2;      // >= floor((u0 + 63 + p) / s) - floor((u0 + p - k + 1) / s) + 1
    if (row > XS_MAX || (long long)CT * ksize > WS_MAX || (long long)Tin + padding + ksize >= 0x3fffffffLL) return ALM_ERR_UNSUPPORTED;
    a.row = (int)row;
    a.chunk = (int)min((long long)a.cog, min(XS_MAX / row, (long long)WS_MAX / (CT * ksize)));
    a.tiles = (a.cig + CT - 1) / CT;
    const long long gy = (long long)groups * a.tiles;
    if (gy > 65535 || B > 65535) return ALM_ERR_UNSUPPORTED;
    const dim3 grid((Tin + TT - 1) / TT, (unsigned)gy, B);
    if (J == 4) hipLaunchKernelGGL(gconv_dgrad_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gconv_dgrad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of alm_gconv1d_wgrad: splits x (numel(dw) + Cout); -1 when the shape is outside the kernel's envelope
extern "C" int alm_gconv1d_wgrad_ws_floats(int B, int Cin, int Cout, int Tin, int ksize, int stride, int padding, int groups) {
    if (!conv_shape_ok(B, Cin, Cout, Tin, ksize, stride, padding, groups)) return -1;
    WgPlan p;
    if (!wgrad_plan(B, Cin, Cout, alm_gconv1d_out_len(Tin, ksize, stride, padding), ksize, stride, groups, p)) return -1;
    const long long n = (long long)p.splits * ((long long)Cout * (Cin / groups) * ksize + Cout);
    return n >= 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_gconv1d_wgrad(const float* g, const float* y, const float* x, float* dw, float* db, float* ws, long long ws_floats, int B, int Cin,
                                 int Cout, int Tin, int ksize, int stride, int padding, int groups, void* stream) {
    if (!conv_shape_ok(B, Cin, Cout, Tin, ksize, stride, padding, groups)) return ALM_ERR_BAD_ARG;
    GConvArgs a = {};
    a.g = g, a.y = y, a.x = x, a.out = ws;
    a.B = B, a.Cin = Cin, a.Cout = Cout, a.Tin = Tin, a.K = ksize, a.s = stride, a.p = padding, a.G = groups, a.act = y != nullptr;
    a.Tout = alm_gconv1d_out_len(Tin, ksize, stride, padding);
    a.cig = Cin / groups, a.cog = Cout / groups;
    WgPlan p;
    if (!wgrad_plan(B, Cin, Cout, a.Tout, ksize, stride, groups, p) || (long long)Tin * stride >= 0x3fffffffLL) return ALM_ERR_UNSUPPORTED;
    const long long ndw = (long long)Cout * a.cig * ksize;
    if (ws_floats < (long long)p.splits * (ndw + Cout)) return ALM_ERR_BAD_ARG;
    a.cot = p.cot, a.cit = p.cit, a.ncot = p.ncot, a.ncit = p.ncit, a.per = p.per, a.nchunk = p.nchunk, a.nT = p.nT, a.row = p.row;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.splits, (unsigned)(groups * p.ncot * p.ncit));
    const int nj = (p.cot * p.cit * ksize + 255) / 256;             // sums per thread
    if (nj <= 1) hipLaunchKernelGGL(gconv_wgrad_kernel<1>, grid, dim3(256), 0, st, a);
    else if (nj <= 2) hipLaunchKernelGGL(gconv_wgrad_kernel<2>, grid, dim3(256), 0, st, a);
    else if (nj <= 5) hipLaunchKernelGGL(gconv_wgrad_kernel<5>, grid, dim3(256), 0, st, a);
    else if (nj <= 8) hipLaunchKernelGGL(gconv_wgrad_kernel<8>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(gconv_wgrad_kernel<WG_ACC>, grid, dim3(256), 0, st, a);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(discr_wgrad_reduce_kernel, dim3((unsigned)((ndw + Cout + 255) / 256)), dim3(256), 0, st, ws, dw, db, ndw, Cout, p.splits);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_avgpool1d_out_len(int T, int f) { return (T <= 0 || f <= 0) ? -1 : T / f + 1; }

extern "C" int alm_avgpool1d_fwd(const float* x, float* y, long long rows, int T, int f, void* stream) {
    if (rows <= 0 || T <= 0 || f <= 0) return ALM_ERR_BAD_ARG;
    const int Tout = T / f + 1;
    const long long n = rows * Tout;
    if ((n + 255) / 256 >= 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, rows, T, Tout, f);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_avgpool1d_bwd(const float* g, float* dx, long long rows, int T, int f, void* stream) {
    if (rows <= 0 || T <= 0 || f <= 0) return ALM_ERR_BAD_ARG;
    const int Tout = T / f + 1;
    const long long n = rows * T;
    if ((n + 255) / 256 >= 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, dx, rows, T, Tout, f);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_loss_ws_floats(void) { return RED_MAX_BLOCKS; }

extern "C" int alm_loss_mean_fwd(const float* a, const float* b, float* out, float* ws, long long n, int mode, void* stream) {
    if (n <= 0 || mode < ALM_LOSS_HINGE_DISCR || mode > ALM_LOSS_L1_COMPLEX || (mode != ALM_LOSS_HINGE_GEN && b == nullptr)) return ALM_ERR_BAD_ARG;
    long long span = RED_SPAN;
    while ((n + span - 1) / span > RED_MAX_BLOCKS) span *= 2;
    const int nparts = (int)((n + span - 1) / span);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_partial_kernel, dim3(nparts), dim3(256), 0, st, a, b, ws, n, span, mode);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, ws, out, nparts, (float)(1.0 / (double)n));
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_loss_mean_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long long n, int mode, void* stream) {
    if (n <= 0 || mode < ALM_LOSS_HINGE_DISCR || mode > ALM_LOSS_L1_COMPLEX || (mode != ALM_LOSS_HINGE_GEN && b == nullptr)) return ALM_ERR_BAD_ARG;
    if ((n + 255) / 256 >= 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, gout, da, db, n,
                       (float)(1.0 / (double)n), mode);
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of alm_grad_penalty_fwd: R rows x the blocks per row; -1 outside the kernel's envelope
extern "C" int alm_grad_penalty_ws_floats(int R, long long n) {
    if (R <= 0 || R > PEN_MAX_ROWS || n <= 0) return -1;
    long long span;
    return R * penalty_parts(n, span);
}

extern "C" int alm_grad_penalty_fwd(const float* G, float* out, float* norms, float* ws, long long ws_floats, int R, long long n, float weight,
                                    float center, void* stream) {
    if (G == nullptr || out == nullptr || norms == nullptr || ws == nullptr || R <= 0 || n <= 0) return ALM_ERR_BAD_ARG;
    if (R > PEN_MAX_ROWS) return ALM_ERR_UNSUPPORTED;
    long long span;
    const int nparts = penalty_parts(n, span);
    if (ws_floats < (long long)R * nparts) return ALM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(penalty_partial_kernel, dim3(nparts, R), dim3(256), 0, st, G, ws, n, span);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(penalty_final_kernel, dim3(1), dim3(256), 0, st, ws, norms, out, R, nparts, (float)((double)weight / (double)R), center);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_grad_penalty_bwd(const float* G, const float* norms, const float* gout, float* dG, int R, long long n, float weight, float center,
                                    void* stream) {
    if (G == nullptr || norms == nullptr || gout == nullptr || dG == nullptr || R <= 0 || n <= 0) return ALM_ERR_BAD_ARG;
    if (R > PEN_MAX_ROWS || (n + 255) / 256 >= 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(penalty_bwd_kernel, dim3((unsigned)((n + 255) / 256), R), dim3(256), 0, (hipStream_t)stream, G, norms, gout, dG, n,
                       (float)((double)weight / (double)R), center);
    ALM_LAUNCH_CHECK();
    return 0;
}
