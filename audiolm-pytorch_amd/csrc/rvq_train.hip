// Train-mode residual VQ (vector-quantize-pytorch GroupedResidualVQ as the reference builds it, soundstream.py:592-607; restated in
// tests/rvq_train_restated.py): per-code statistics, the row-local quantize step (commit loss, rotation trick / straight-through), the EMA codebook
// update with Laplace smoothing, dead-code expiry, the k-means means update and the backward.  fp32 throughout, NO float atomics: every output is a
// fixed function of its inputs, bitwise reproducible run to run.  The assignment itself (argmin) stays on alm_rvq_encode (csrc/codec.hip).
//
//   alm_rvq_code_stats : n[c] = #rows with idx == c, s[c] = their sum.  The reference forms this as a dense one-hot GEMM (2 C M d flop); here it is a
//       segment sum that touches every row once.  Destination-owned, five small launches:
//         (1) per tile of ST_TILE rows, a histogram of the codes in LDS (integer atomics: exact, hence deterministic)        -> hist[tile][C]
//         (2) one workgroup: per code an exclusive scan over the tiles (in place), the counts, and the exclusive scans over the codes of the
//             row counts (cstart) and of the chunk counts ceil(n_c / ST_CH) (kstart)
//         (3) per tile: every row's slot = cstart[c] + hist[tile][c] + (rows of the same code before it in the tile)        -> perm: a STABLE
//             counting sort, a code's rows are listed in ascending row order
//         (4) one workgroup per CHUNK of ST_CH listed rows of one code (binary search of the chunk id in kstart): sums them in list order -> partial
//         (5) one workgroup per code: adds its chunks' partials in chunk order and writes s (zero for a code without rows)
//       A collapsed codebook (most rows on a few codes: the normal state early in training) spreads over M / ST_CH workgroups in (4); only the short
//       chain of (5) is serial per code.  Nothing depends on scheduling.  embed_ce.hip's alm_embed_scatter_owned is the precedent (owner + hot-row
//       split); it scans token ranges of several tables at once and shares no code with this sort-based form.
//   alm_rvq_train_quantize / alm_rvq_train_bwd / alm_rvq_expire : one wave per row, the row in registers (d <= 1024: lane l holds columns l + 64 k).
//       All three go through rvq_row_y, written with explicit roundings (no contraction freedom), so the backward's and the expiry's recomputed
//       residual chain is bit-identical to the forward's.
#include "common.hpp"

#pragma clang fp contract(off)           // only the fmas that are written out: rvq_row_y must give the same bits in every kernel that inlines it

namespace {

// The pragma reaches only operations written in THIS file.  The HIP headers' __fmul_rn / __fadd_rn / __fsub_rn are a plain `*`, `+`, `-` compiled under
// the header's own contraction mode (hipcc's default, fast): once inlined their results still carry the `contract` flag, and the backend fused them
// into fmas of its choosing, differently in every kernel (u + qh became fma(r, 1 / |r|, qh): not 0 for r = -2 q, and rvq_expire's bits were not
// rvq_train_quantize's at 4 and more columns per lane; caught by tests/test_gpu_rvq_train_kernels.py).  Hence the single roundings are spelled here.
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int ST_TILE = 256;            // rows per histogram / scatter tile (= threads per workgroup)
constexpr int ST_CH = 64;                // rows per chunk of a code's row list
constexpr int ST_CMAX = 8192;            // codes at most (LDS histogram: 32 KB)

__global__ __launch_bounds__(256) void stats_hist_kernel(const long long* __restrict__ idx, long long ldi, int* __restrict__ hist, int M, int C) {
    extern __shared__ int sh_hist[];
    for (int c = threadIdx.x; c < C; c += 256) sh_hist[c] = 0;
    __syncthreads();
    const long long row = (long long)blockIdx.x * ST_TILE + threadIdx.x;
    if (row < M) {
        const long long c = idx[row * ldi];
        if (c >= 0 && c < C) atomicAdd(&sh_hist[(int)c], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) hist[(long long)blockIdx.x * C + c] = sh_hist[c];
}

// one workgroup.  Thread t owns the codes [t * per, (t + 1) * per).
__global__ __launch_bounds__(256) void stats_scan_kernel(int* __restrict__ hist, int* __restrict__ cstart, int* __restrict__ kstart, float* __restrict__ n_out,
                                                         int ntiles, int C) {
    __shared__ int sh_rows[256], sh_chunks[256];
    const int per = (C + 255) / 256;
    const int c0 = min(C, (int)threadIdx.x * per), c1 = min(C, c0 + per);
    int trows = 0, tchunks = 0;
    for (int c = c0; c < c1; ++c) {
        int run = 0;
        for (int t = 0; t < ntiles; ++t) {
            const long long o = (long long)t * C + c;
            const int v = hist[o];
            hist[o] = run;
            run += v;
        }
        n_out[c] = (float)run;
        cstart[c] = run;                                              // the count for now; the offset below
        trows += run;
        tchunks += (run + ST_CH - 1) / ST_CH;
    }
    sh_rows[threadIdx.x] = trows;
    sh_chunks[threadIdx.x] = tchunks;
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0, k = 0;
        for (int t = 0; t < 256; ++t) {
            const int a = sh_rows[t], b = sh_chunks[t];
            sh_rows[t] = r, sh_chunks[t] = k;
            r += a, k += b;
        }
        cstart[C] = r, kstart[C] = k;
    }
    __syncthreads();
    int r = sh_rows[threadIdx.x], k = sh_chunks[threadIdx.x];
    for (int c = c0; c < c1; ++c) {
        const int cnt = cstart[c];
        cstart[c] = r, kstart[c] = k;
        r += cnt, k += (cnt + ST_CH - 1) / ST_CH;
    }
}

__global__ __launch_bounds__(256) void stats_scatter_kernel(const long long* __restrict__ idx, long long ldi, const int* __restrict__ hist,
                                                            const int* __restrict__ cstart, int* __restrict__ perm, int M, int C) {
    __shared__ int sh_code[ST_TILE];
    const long long row = (long long)blockIdx.x * ST_TILE + threadIdx.x;
    int c = -1;
    if (row < M) {
        const long long v = idx[row * ldi];
        if (v >= 0 && v < C) c = (int)v;
    }
    sh_code[threadIdx.x] = c;
    __syncthreads();
    if (c < 0) return;
    int rank = 0;
    for (int j = 0; j < (int)threadIdx.x; ++j) rank += sh_code[j] == c;
    const int pos = cstart[c] + hist[(long long)blockIdx.x * C + c] + rank;
    if (pos >= 0 && pos < M) perm[pos] = (int)row;
}

// grid (chunk slots, column blocks of 256).  chunk j belongs to the code c with kstart[c] <= j < kstart[c + 1].
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* __restrict__ r, long long ldr, const int* __restrict__ perm,
                                                            const int* __restrict__ cstart, const int* __restrict__ kstart, float* __restrict__ partial, int M, int d,
                                                            int C) {
    __shared__ int sh_rows[ST_CH];
    const int j = blockIdx.x;
    if (j >= kstart[C]) return;
    int lo = 0, hi = C;                                               // first c with kstart[c] > j, minus one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kstart[mid] <= j) lo = mid + 1; else hi = mid;
    }
    const int c = lo - 1;
    const int base = cstart[c] + (j - kstart[c]) * ST_CH;
    const int cnt = min(ST_CH, cstart[c + 1] - base);
    if ((int)threadIdx.x < cnt) sh_rows[threadIdx.x] = perm[base + threadIdx.x];
    __syncthreads();
    const int col = blockIdx.y * 256 + threadIdx.x;
    if (col >= d) return;
    float acc = 0.f;
    int i = 0;
    for (; i + 8 <= cnt; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = r[(long long)sh_rows[i + u] * ldr + col];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; i < cnt; ++i) acc += r[(long long)sh_rows[i] * ldr + col];
    partial[(long long)j * d + col] = acc;
}

__global__ __launch_bounds__(256) void stats_final_kernel(const float* __restrict__ partial, const int* __restrict__ kstart, float* __restrict__ s, int d, int C) {
    const int c = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (c >= C || col >= d) return;
    const int k0 = kstart[c], k1 = kstart[c + 1];
    float acc = 0.f;
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = partial[(long long)(k + u) * d + col];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; k < k1; ++k) acc += partial[(long long)k * d + col];
    s[(long long)c * d + col] = acc;
}

// ---- the row-local step.  Lane l of the wave holds columns l + 64 k (zero beyond d); every sum is the lane's fma chain over k, then the xor butterfly
// (the same tree in every lane: all lanes hold the same bits).  Explicit roundings only, so every caller computes the same bits.
template <int K>
struct RvqRow {
    float u[K], qh[K], w[K];
    float lam;
};

template <int K>
__device__ __forceinline__ float row_dot(const float (&a)[K], const float (&b)[K]) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) acc = __fmaf_rn(a[k], b[k], acc);
    return wave_sum(acc);
}

// y of one layer from its residual r and the selected code q.  rotation: rotate_to(r, q) with u = r / |r|, qh = q / |q| (0 where the norm is 0),
// w = (u + qh) / max(|u + qh|, 1e-12), lam = |q| / |r| (0 where |r| is 0):  y = lam (r - 2 (r.w) w + 2 (r.u) qh).  else y = r + (q - r).
template <int K>
__device__ __forceinline__ void rvq_row_y(const float (&r)[K], const float (&q)[K], int rotation, float (&y)[K], RvqRow<K>& s) {
    if (!rotation) {
#pragma unroll
        for (int k = 0; k < K; ++k) y[k] = add_rn(r[k], sub_rn(q[k], r[k]));
        return;
    }
    const float rn = __fsqrt_rn(row_dot<K>(r, r)), qn = __fsqrt_rn(row_dot<K>(q, q));
    const float inv_r = rn > 0.f ? __fdiv_rn(1.f, rn) : 0.f, inv_q = qn > 0.f ? __fdiv_rn(1.f, qn) : 0.f;
    float t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s.u[k] = mul_rn(r[k], inv_r);
        s.qh[k] = mul_rn(q[k], inv_q);
        t[k] = add_rn(s.u[k], s.qh[k]);
    }
    const float inv_t = __fdiv_rn(1.f, fmaxf(__fsqrt_rn(row_dot<K>(t, t)), 1e-12f));
#pragma unroll
    for (int k = 0; k < K; ++k) s.w[k] = mul_rn(t[k], inv_t);
    const float rw2 = mul_rn(2.f, row_dot<K>(r, s.w)), ru2 = mul_rn(2.f, row_dot<K>(r, s.u));
    s.lam = mul_rn(qn, inv_r);
#pragma unroll
    for (int k = 0; k < K; ++k) y[k] = mul_rn(s.lam, __fmaf_rn(ru2, s.qh[k], __fmaf_rn(-rw2, s.w[k], r[k])));
}

template <int K>
__device__ __forceinline__ void row_load(float (&v)[K], const float* __restrict__ p, int lane, int d) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = lane + 64 * k;
        v[k] = e < d ? p[e] : 0.f;
    }
}

constexpr int TQ_ROWS = 32;              // rows per workgroup of the forward step: 4 waves x 8 rows, one loss partial per workgroup

template <int K>
__global__ __launch_bounds__(256) void rvq_train_quantize_kernel(float* __restrict__ resid, long long ldr, const long long* __restrict__ idx, long long ldi,
                                                                 const float* __restrict__ E, float* __restrict__ out, long long ldo, float* __restrict__ part,
                                                                 int rotation, int M, int d, int C) {
    __shared__ float sh_loss[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float lsum = 0.f;
    for (int j = 0; j < TQ_ROWS / 4; ++j) {
        const long long row = (long long)blockIdx.x * TQ_ROWS + wave * (TQ_ROWS / 4) + j;
        if (row >= M) break;
        const long long c = idx[row * ldi];
        if (c < 0 || c >= C) continue;
        float r[K], q[K], y[K], df[K];
        RvqRow<K> s;
        row_load<K>(r, resid + row * ldr, lane, d);
        row_load<K>(q, E + c * d, lane, d);
#pragma unroll
        for (int k = 0; k < K; ++k) df[k] = sub_rn(q[k], r[k]);
        lsum = add_rn(lsum, row_dot<K>(df, df));
        rvq_row_y<K>(r, q, rotation, y, s);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = lane + 64 * k;
            if (e < d) {
                resid[row * ldr + e] = sub_rn(r[k], y[k]);
                out[row * ldo + e] = add_rn(out[row * ldo + e], y[k]);
            }
        }
    }
    if (lane == 0) sh_loss[wave] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = add_rn(add_rn(add_rn(sh_loss[0], sh_loss[1]), sh_loss[2]), sh_loss[3]);
}

// fixed-order sum of n floats by one workgroup: thread t adds elements t, t + 256, ... in order, then a fixed LDS tree.  (every thread returns the total)
__device__ __forceinline__ float block_sum_fixed(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = add_rn(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    const float total = sh[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(256) void rvq_loss_finish_kernel(const float* __restrict__ part, int n, float scale, float* __restrict__ loss) {
    __shared__ float sh[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc = add_rn(acc, part[i]);
    const float total = block_sum_fixed(acc, sh);
    if (threadIdx.x == 0) loss[0] = mul_rn(total, scale);
}

// one workgroup: cluster_size = cluster_size * decay + n * (1 - decay), its sum over the codes in a fixed order, and the ascending list of the
// codes that fall below `threshold` (dead[0] = their number, dead[1 ...] = the codes; threshold <= 0: none).
__global__ __launch_bounds__(256) void rvq_ema_size_kernel(float* __restrict__ cluster_size, const float* __restrict__ n, float decay, float threshold,
                                                           int* __restrict__ dead, float* __restrict__ total, int C) {
    __shared__ float sh[256];
    __shared__ int sh_cnt[4];
    __shared__ int sh_base;
    float acc = 0.f;
    if (threadIdx.x == 0) sh_base = 0;
    const float om = 1.f - decay;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < C; c0 += 256) {
        const int c = c0 + threadIdx.x;
        bool is_dead = false;
        if (c < C) {
            const float v = __fmaf_rn(cluster_size[c], decay, mul_rn(n[c], om));
            cluster_size[c] = v;
            acc = add_rn(acc, v);
            is_dead = threshold > 0.f && v < threshold;
        }
        const unsigned long long bal = __ballot(is_dead);
        if (lane == 0) sh_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = sh_base;
        for (int w = 0; w < wave; ++w) off += sh_cnt[w];
        if (is_dead) dead[1 + off + __popcll(bal & ((1ull << lane) - 1ull))] = c;
        __syncthreads();
        if (threadIdx.x == 0) sh_base += sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
        __syncthreads();
    }
    const float t = block_sum_fixed(acc, sh);
    if (threadIdx.x == 0) {
        total[0] = t;
        dead[0] = sh_base;
    }
}

// grid (C, column blocks): embed_avg = embed_avg * decay + s * (1 - decay); embed = embed_avg / smoothed, smoothed = (cs + eps) / (sum + C eps) * sum
__global__ __launch_bounds__(256) void rvq_ema_embed_kernel(const float* __restrict__ cluster_size, float* __restrict__ embed_avg, float* __restrict__ embed,
                                                            const float* __restrict__ s, const float* __restrict__ total, float decay, float eps, int C, int d) {
    const int c = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (c >= C || col >= d) return;
    const float tot = total[0];
    const float smoothed = mul_rn(__fdiv_rn(add_rn(cluster_size[c], eps), __fmaf_rn((float)C, eps, tot)), tot);
    const long long o = (long long)c * d + col;
    const float ea = __fmaf_rn(embed_avg[o], decay, mul_rn(s[o], 1.f - decay));
    embed_avg[o] = ea;
    embed[o] = __fdiv_rn(ea, smoothed);
}

// grid = listed codes, one wave each: the layer-q residual of the sampled row, recomputed from x, the saved indices and the pre-update codebooks
template <int K>
__global__ __launch_bounds__(64) void rvq_expire_kernel(const int* __restrict__ dead, int count, const long long* __restrict__ rows, const float* __restrict__ x,
                                                        long long ldx, const long long* __restrict__ idx, long long ldi, const float* __restrict__ E, int q,
                                                        int rotation, float threshold, float* __restrict__ cluster_size, float* __restrict__ embed_avg,
                                                        float* __restrict__ embed, int M, int d, int C) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const int code = dead[i];
    const long long row = rows[i];
    if (code < 0 || code >= C || row < 0 || row >= M) return;
    float r[K];
    row_load<K>(r, x + row * ldx, lane, d);
    for (int l = 0; l < q; ++l) {
        const long long c = idx[row * ldi + l];
        if (c < 0 || c >= C) continue;
        float e[K], y[K];
        RvqRow<K> s;
        row_load<K>(e, E + ((long long)l * C + c) * d, lane, d);
        rvq_row_y<K>(r, e, rotation, y, s);
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = sub_rn(r[k], y[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = lane + 64 * k;
        if (e < d) {
            embed[(long long)code * d + e] = r[k];
            embed_avg[(long long)code * d + e] = mul_rn(r[k], threshold);
        }
    }
    if (lane == 0) cluster_size[code] = threshold;
}

// grid (C, column blocks): means = bins == 0 ? means : s / max(bins, 1); with `embed` also the final copy embed = means, embed_avg = means * bins,
// cluster_size = bins
__global__ __launch_bounds__(256) void rvq_kmeans_kernel(float* __restrict__ means, const float* __restrict__ n, const float* __restrict__ s, float* __restrict__ embed,
                                                         float* __restrict__ embed_avg, float* __restrict__ cluster_size, int C, int d) {
    const int c = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (c >= C || col >= d) return;
    const float bins = n[c];
    const long long o = (long long)c * d + col;
    const float m = bins == 0.f ? means[o] : __fdiv_rn(s[o], fmaxf(bins, 1.f));
    means[o] = m;
    if (embed != nullptr) {
        embed[o] = m;
        embed_avg[o] = mul_rn(m, bins);
        if (col == 0) cluster_size[c] = bins;
    }
}

// one wave per row: the row's chain over the Q layers recomputed from x, idx and the pre-update codebooks;
// dx = sum_q [ (dy_q / dr)^T g + coef_q (r_q - quant_q) ],  (dy/dr)^T g = lam (g - 2 (w.g) w + 2 (qh.g) u)  (straight-through: g)
template <int K>
__global__ __launch_bounds__(256) void rvq_train_bwd_kernel(const float* __restrict__ x, long long ldx, const long long* __restrict__ idx, long long ldi,
                                                            const float* __restrict__ E, const float* __restrict__ g_out, long long ldg,
                                                            const float* __restrict__ coef, float* __restrict__ dx, long long lddx, int rotation, int M, int d, int C,
                                                            int Q) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float r[K], g[K], acc[K];
    row_load<K>(r, x + row * ldx, lane, d);
    if (g_out != nullptr) row_load<K>(g, g_out + row * ldg, lane, d);
    else {
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int l = 0; l < Q; ++l) {
        const long long c = idx[row * ldi + l];
        if (c < 0 || c >= C) continue;
        float e[K], y[K];
        RvqRow<K> s;
        row_load<K>(e, E + ((long long)l * C + c) * d, lane, d);
        rvq_row_y<K>(r, e, rotation, y, s);
        const float cf = coef != nullptr ? coef[l] : 0.f;
        if (rotation) {
            const float wg2 = mul_rn(2.f, row_dot<K>(s.w, g)), qg2 = mul_rn(2.f, row_dot<K>(s.qh, g));
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = add_rn(acc[k], mul_rn(s.lam, __fmaf_rn(qg2, s.u[k], __fmaf_rn(-wg2, s.w[k], g[k]))));
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = add_rn(acc[k], g[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            acc[k] = __fmaf_rn(cf, sub_rn(r[k], e[k]), acc[k]);
            r[k] = sub_rn(r[k], y[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = lane + 64 * k;
        if (e < d) dx[row * lddx + e] = acc[k];
    }
}

inline int row_k(int d) { return d <= 64 ? 1 : d <= 128 ? 2 : d <= 256 ? 4 : d <= 512 ? 8 : d <= 1024 ? 16 : 0; }

#define RVQ_ROW_DISPATCH(K_, LAUNCH)                  \
    switch (K_) {                                     \
        case 1: { constexpr int K = 1; LAUNCH; } break;   \
        case 2: { constexpr int K = 2; LAUNCH; } break;   \
        case 4: { constexpr int K = 4; LAUNCH; } break;   \
        case 8: { constexpr int K = 8; LAUNCH; } break;   \
        default: { constexpr int K = 16; LAUNCH; } break; \
    }

inline long long stats_chunk_slots(int M, int C) { return (long long)M / ST_CH + C; }   // >= sum_c ceil(n_c / ST_CH)

}  // namespace

extern "C" int alm_rvq_code_stats_chunk(void) { return ST_CH; }

// workspace of alm_rvq_code_stats in floats (4-byte words): hist [tiles][C] | cstart [C + 1] | kstart [C + 1] | perm [M] | partial [chunk slots][d];
// -1 when it does not fit an int
extern "C" int alm_rvq_code_stats_ws_floats(int M, int d, int C) {
    if (M < 0 || d <= 0 || C <= 0) return -1;
    const long long tiles = ((long long)M + ST_TILE - 1) / ST_TILE;
    const long long w = tiles * C + 2ll * (C + 1) + M + stats_chunk_slots(M, C) * d;
    return w > 0x7fffffffll ? -1 : (int)w;
}

extern "C" int alm_rvq_code_stats(const float* r, long long ldr, const long long* idx, long long ldi, float* n, float* s, float* ws, long long ws_floats,
                                  int M, int d, int C, void* stream) {
    if (M < 0 || d <= 0 || C <= 0 || ldr < d || ldi < 1 || n == nullptr || s == nullptr) return ALM_ERR_BAD_ARG;
    if (C > ST_CMAX) return ALM_ERR_UNSUPPORTED;
    const int need = alm_rvq_code_stats_ws_floats(M, d, C);
    if (need < 0) return ALM_ERR_UNSUPPORTED;
    if (ws == nullptr || ws_floats < need) return ALM_ERR_BAD_ARG;
    const int tiles = (M + ST_TILE - 1) / ST_TILE;
    int* hist = reinterpret_cast<int*>(ws);
    int* cstart = hist + (long long)tiles * C;
    int* kstart = cstart + C + 1;
    int* perm = kstart + C + 1;
    float* partial = reinterpret_cast<float*>(perm + M);
    hipStream_t st = (hipStream_t)stream;
    const unsigned dy = (unsigned)((d + 255) / 256);
    if (tiles > 0) hipLaunchKernelGGL(stats_hist_kernel, dim3((unsigned)tiles), dim3(256), (size_t)C * sizeof(int), st, idx, ldi, hist, M, C);
    hipLaunchKernelGGL(stats_scan_kernel, dim3(1), dim3(256), 0, st, hist, cstart, kstart, n, tiles, C);
    if (tiles > 0) {
        hipLaunchKernelGGL(stats_scatter_kernel, dim3((unsigned)tiles), dim3(256), 0, st, idx, ldi, hist, cstart, perm, M, C);
        hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)stats_chunk_slots(M, C), dy), dim3(256), 0, st, r, ldr, perm, cstart, kstart, partial, M, d, C);
    }
    hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)C, dy), dim3(256), 0, st, partial, kstart, s, d, C);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_rvq_train_quantize_blocks(int M) { return M <= 0 ? 0 : (M + TQ_ROWS - 1) / TQ_ROWS; }

extern "C" int alm_rvq_train_quantize(float* resid, long long ldr, const long long* idx, long long ldi, const float* E, float* out, long long ldo, float* loss,
                                      float* part, float loss_scale, int rotation, int M, int d, int C, void* stream) {
    if (M <= 0 || d <= 0 || C <= 0 || ldr < d || ldo < d || ldi < 1 || loss == nullptr || part == nullptr) return ALM_ERR_BAD_ARG;
    const int k = row_k(d);
    if (k == 0) return ALM_ERR_UNSUPPORTED;
    const int blocks = alm_rvq_train_quantize_blocks(M);
    hipStream_t st = (hipStream_t)stream;
    RVQ_ROW_DISPATCH(k, hipLaunchKernelGGL(rvq_train_quantize_kernel<K>, dim3((unsigned)blocks), dim3(256), 0, st, resid, ldr, idx, ldi, E, out, ldo, part, rotation,
                                           M, d, C));
    hipLaunchKernelGGL(rvq_loss_finish_kernel, dim3(1), dim3(256), 0, st, part, blocks, loss_scale, loss);
    ALM_LAUNCH_CHECK();
    return 0;
}

// dead: int [1 + C] (count, then the codes below `threshold` in ascending order); total: one float of workspace
extern "C" int alm_rvq_ema_update(float* cluster_size, float* embed_avg, float* embed, const float* n, const float* s, float decay, float eps, float threshold,
                                  int* dead, float* total, int C, int d, void* stream) {
    if (C <= 0 || d <= 0 || dead == nullptr || total == nullptr) return ALM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rvq_ema_size_kernel, dim3(1), dim3(256), 0, st, cluster_size, n, decay, threshold, dead, total, C);
    hipLaunchKernelGGL(rvq_ema_embed_kernel, dim3((unsigned)C, (unsigned)((d + 255) / 256)), dim3(256), 0, st, cluster_size, embed_avg, embed, s, total, decay, eps, C,
                       d);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_rvq_expire(const int* dead, int count, const long long* rows, const float* x, long long ldx, const long long* idx, long long ldi, const float* E,
                              int q, int rotation, float threshold, float* cluster_size, float* embed_avg, float* embed, int M, int d, int C, void* stream) {
    if (count < 0 || count > C || M <= 0 || d <= 0 || C <= 0 || q < 0 || ldx < d || ldi < q) return ALM_ERR_BAD_ARG;
    const int k = row_k(d);
    if (k == 0) return ALM_ERR_UNSUPPORTED;
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    RVQ_ROW_DISPATCH(k, hipLaunchKernelGGL(rvq_expire_kernel<K>, dim3((unsigned)count), dim3(64), 0, st, dead, count, rows, x, ldx, idx, ldi, E, q, rotation, threshold,
                                           cluster_size, embed_avg, embed, M, d, C));
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_rvq_kmeans_update(float* means, const float* n, const float* s, float* embed, float* embed_avg, float* cluster_size, int C, int d, void* stream) {
    if (C <= 0 || d <= 0 || (embed != nullptr && (embed_avg == nullptr || cluster_size == nullptr))) return ALM_ERR_BAD_ARG;
    hipLaunchKernelGGL(rvq_kmeans_kernel, dim3((unsigned)C, (unsigned)((d + 255) / 256)), dim3(256), 0, (hipStream_t)stream, means, n, s, embed, embed_avg,
                       cluster_size, C, d);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_rvq_train_bwd(const float* x, long long ldx, const long long* idx, long long ldi, const float* E, const float* g_out, long long ldg,
                                 const float* coef, float* dx, long long lddx, int rotation, int M, int d, int C, int Q, void* stream) {
    if (M <= 0 || d <= 0 || C <= 0 || Q <= 0 || ldx < d || lddx < d || ldi < Q || (g_out != nullptr && ldg < d)) return ALM_ERR_BAD_ARG;
    const int k = row_k(d);
    if (k == 0) return ALM_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    RVQ_ROW_DISPATCH(k, hipLaunchKernelGGL(rvq_train_bwd_kernel<K>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, ldx, idx, ldi, E, g_out, ldg, coef, dx, lddx,
                                           rotation, M, d, C, Q));
    ALM_LAUNCH_CHECK();
    return 0;
}
