// vq-wav2vec with the k-means quantizer (fairseq models/wav2vec/wav2vec.py: Wav2VecModel, ConvFeatureExtractionModel, KmeansVectorQuantizer; what the
// reference's vq_wav2vec.py:19-81 calls) on gfx950, fp32 throughout, activations [B][C][T].  The convolutions and the code search are the shared
// alm_conv1d_valid / alm_rvq_encode; new here is the normalisation: GroupNorm(1, C) after EVERY conv layer and GroupNorm(groups, C) in the quantizer
// head, so each id depends on statistics over a whole clip.  No atomics anywhere: every number is one fixed-order chain, bitwise reproducible.
//
//   group statistics : (mean, rstd) of the contiguous (C / G) x T block of a sample's group.  Stage 1: a workgroup per chunk of GS_CHUNK = 4096
//                      elements, held in registers (16 per thread): the chunk mean, then the sums of d = x - mean and d^2 about it, so that
//                      M2 = sum d^2 - (sum d)^2 / n never cancels (the sum d term only corrects the rounding of the mean).  Each level sums
//                      16 terms per thread, 6 shuffle levels per wave, 4 waves.  Stage 2: a workgroup per (sample, group) merges the partials by
//                      Chan's update in fp64, thread i a contiguous run of them in index order, then a fixed pairwise tree over the 256 threads.
//   layer 0          : Cin = 1 and the largest activation, never stored un-normalised: the per-(row, channel, chunk) partials of conv0_stats.hpp
//                      (shared with hubert.hip) go through the same stage 2, then the conv is recomputed and ReLU(GN(.)) written once.
//   apply            : layers >= 1, in place on the raw conv output: gamma (x - mean) rstd + beta, ReLU, optional skip (x + r[t * rstep]) * scale,
//                      optional log(|x| + 1).
//   apply transposed : the quantizer head, normalised and stored [B][T][C] so that each group's rows are unit-stride for the code search.
#include "common.hpp"
#include "conv0_stats.hpp"

namespace {

constexpr int GS_CHUNK = 4096;        // elements per statistics chunk: 256 threads x 16 registers
constexpr int GS_PER = GS_CHUNK / 256;

// ---- stage 1: part[bg][chunk] = (mean, M2) of elements [chunk * GS_CHUNK, ...) of the block x + bg * L ----
__global__ __launch_bounds__(256) void group_part_kernel(const float* __restrict__ x, float2* __restrict__ part, long long L, int chunks) {
    const int chunk = blockIdx.x;
    const long long bg = blockIdx.y;
    const long long e0 = (long long)chunk * GS_CHUNK;
    const int n = (int)min((long long)GS_CHUNK, L - e0);
    const float* src = x + (size_t)bg * L + e0;
    float v[GS_PER];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < GS_PER; ++j) {
        const int i = j * 256 + threadIdx.x;
        v[j] = i < n ? src[i] : 0.f;
        s += v[j];
    }
    const float m0 = block_sum(s) / (float)n;
    float sd = 0.f, q = 0.f;
#pragma unroll
    for (int j = 0; j < GS_PER; ++j) {
        const float d = (j * 256 + (int)threadIdx.x) < n ? v[j] - m0 : 0.f;
        sd += d;
        q = fmaf(d, d, q);
    }
    sd = block_sum(sd);
    q = block_sum(q);
    if (threadIdx.x == 0) {
        const float md = sd / (float)n;
        part[(size_t)bg * chunks + chunk] = make_float2(m0 + md, fmaxf(q - sd * md, 0.f));
    }
}

// Chan et al.: (n, mean, M2) <- (n, mean, M2) merged with (nb, mb, M2b)
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& M2, double nb, double mb, double M2b) {
    if (nb == 0.) return;
    const double tot = n + nb, delta = mb - mean;
    mean += delta * (nb / tot);
    M2 += M2b + delta * delta * (n * nb / tot);
    n = tot;
}

// ---- stage 2: stats[bg] = (mean, rstd) from the P partials part[bg][0 .. P), biased variance as nn.GroupNorm.  Partial p covers
// min(chunk, row_len - (p % cpr) * chunk) elements: rows of cpr chunks (layer 0: a row per channel; the generic statistics: one row, cpr = P). ----
__global__ __launch_bounds__(256) void group_merge_kernel(const float2* __restrict__ part, float2* __restrict__ stats, long long P, int cpr,
                                                          long long row_len, int chunk, float eps) {
    __shared__ double sn[256], sm[256], sq[256];
    const long long bg = blockIdx.x;
    const float2* src = part + (size_t)bg * P;
    const long long per = (P + 255) / 256;
    const long long p0 = per * threadIdx.x, p1 = min(p0 + per, P);
    double n = 0., mean = 0., M2 = 0.;
    for (long long p = p0; p < p1; ++p) {
        const float2 v = src[p];
        const double nb = (double)min((long long)chunk, row_len - (p % cpr) * chunk);
        chan_merge(n, mean, M2, nb, (double)v.x, (double)v.y);
    }
    sn[threadIdx.x] = n, sm[threadIdx.x] = mean, sq[threadIdx.x] = M2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            chan_merge(n, mean, M2, sn[threadIdx.x + s], sm[threadIdx.x + s], sq[threadIdx.x + s]);
            sn[threadIdx.x] = n, sm[threadIdx.x] = mean, sq[threadIdx.x] = M2;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) stats[bg] = make_float2((float)mean, (float)(1.0 / sqrt(M2 / n + (double)eps)));
}

struct GnApplyArgs {
    float* x;                   // [B][C][T], in place
    const float2* stats;        // [B][G]
    const float *gamma, *beta;  // [C]
    const float* residual;      // [B][C][r_T] or NULL
    int C, T, cpg, r_T, rstep, relu, logc;
    float scale;
};

// ---- apply, in place; a thread takes 4 elements 256 apart of one sample's C x T block ----
__global__ __launch_bounds__(256) void gn_apply_kernel(const GnApplyArgs a) {
    const long long b = blockIdx.y;
    const long long CT = (long long)a.C * a.T;
    float* xb = a.x + (size_t)b * CT;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = (long long)blockIdx.x * 1024 + j * 256 + threadIdx.x;
        if (i >= CT) return;
        const int c = (int)(i / a.T), t = (int)(i - (long long)c * a.T);
        const float2 s = a.stats[b * (a.C / a.cpg) + c / a.cpg];
        float v = (xb[i] - s.x) * s.y * a.gamma[c] + a.beta[c];
        if (a.relu) v = fmaxf(v, 0.f);
        if (a.residual) v = (v + a.residual[((size_t)b * a.C + c) * a.r_T + (size_t)t * a.rstep]) * a.scale;
        if (a.logc) v = log1pf(fabsf(v));
        xb[i] = v;
    }
}

// ---- apply transposed: out[b][t][c] = gamma (x[b][c][t] - mean) rstd + beta through a 32 x 32 LDS tile ----
__global__ __launch_bounds__(256) void gn_apply_t_kernel(const float* __restrict__ x, const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ out, int C, int T, int cpg) {
    __shared__ float tile[32][33];
    const long long b = blockIdx.z;
    const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float* xb = x + (size_t)b * C * T;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + ly + 8 * r, t = t0 + lx;
        if (c < C && t < T) {
            const float2 s = stats[b * (C / cpg) + c / cpg];
            tile[ly + 8 * r][lx] = (xb[(size_t)c * T + t] - s.x) * s.y * gamma[c] + beta[c];
        }
    }
    __syncthreads();
    float* ob = out + (size_t)b * T * C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + ly + 8 * r, c = c0 + lx;
        if (c < C && t < T) ob[(size_t)t * C + c] = tile[lx][ly + 8 * r];
    }
}

// layer 0 apply (conv0_stats.hpp): one (mean, rstd) per row, ReLU, optional log(|x| + 1) (a one-layer extractor)
struct Conv0PerRowRelu {
    const float2* __restrict__ stats;
    int logc;
    __device__ __forceinline__ float2 stat(int b, int) const { return stats[b]; }
    __device__ __forceinline__ float act(float v) const {
        v = fmaxf(v, 0.f);
        return logc ? log1pf(v) : v;
    }
};

inline long long gs_chunks(long long L) { return (L + GS_CHUNK - 1) / GS_CHUNK; }

// C x T (and with it every in-group index) fits 32 bits; sample and group offsets are 64-bit
inline int gn_check(int B, int C, int T, int G) {
    if (B <= 0 || C <= 0 || T <= 0 || G <= 0 || C % G) return ALM_ERR_BAD_ARG;
    if ((long long)C * T >= (1LL << 31) - 1024 || (long long)B * G > 65535 || C > 65535 * 32) return ALM_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int alm_vqw2v_group_chunks(int C, int T, int G) {
    if (C <= 0 || T <= 0 || G <= 0 || C % G || (long long)C * T >= (1LL << 31) - 1024) return -1;
    return (int)gs_chunks((long long)(C / G) * T);
}

extern "C" int alm_vqw2v_group_stats(const float* x, float* part, float* stats, int B, int C, int T, int G, float eps, void* stream) {
    if (const int rc = gn_check(B, C, T, G)) return rc;
    const long long L = (long long)(C / G) * T;
    const int chunks = (int)gs_chunks(L);
    hipLaunchKernelGGL(group_part_kernel, dim3(chunks, B * G), dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<float2*>(part), L, chunks);
    hipLaunchKernelGGL(group_merge_kernel, dim3(B * G), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(part),
                       reinterpret_cast<float2*>(stats), (long long)chunks, chunks, L, GS_CHUNK, eps);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_vqw2v_group_apply(float* x, const float* stats, const float* gamma, const float* beta, const float* residual, int B, int C, int T, int G,
                                     int r_T, int rstep, float scale, int relu, int logc, void* stream) {
    if (const int rc = gn_check(B, C, T, G)) return rc;
    if (residual && (rstep <= 0 || r_T <= 0 || (long long)(T - 1) * rstep >= r_T)) return ALM_ERR_BAD_ARG;
    const GnApplyArgs a{x, reinterpret_cast<const float2*>(stats), gamma, beta, residual, C, T, C / G, r_T, rstep, relu, logc, scale};
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)(((long long)C * T + 1023) / 1024), B), dim3(256), 0, (hipStream_t)stream, a);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_vqw2v_group_apply_t(const float* x, const float* stats, const float* gamma, const float* beta, float* out, int B, int C, int T, int G,
                                       void* stream) {
    if (const int rc = gn_check(B, C, T, G)) return rc;
    hipLaunchKernelGGL(gn_apply_t_kernel, dim3((T + 31) / 32, (C + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<const float2*>(stats), gamma, beta, out, C, T, C / G);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_vqw2v_conv0_stats(const float* wave, long long ld_wave, const float* w, float* part, float* stats, int B, int C, long long Tin,
                                     long long Tout, int ksize, int stride, float eps, void* stream) {
    if (const int rc = conv0_check(B, C, Tin, Tout, ksize, stride, ld_wave)) return rc;
    if ((long long)C * Tout >= (1LL << 31) - 1024) return ALM_ERR_UNSUPPORTED;
    const int chunks = conv0_chunks(Tout);
    conv0_stats_launch(wave, ld_wave, w, reinterpret_cast<float2*>(part), B, C, Tin, Tout, ksize, stride, (hipStream_t)stream);
    hipLaunchKernelGGL(group_merge_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(part),
                       reinterpret_cast<float2*>(stats), (long long)C * chunks, chunks, Tout, C0_CHUNK, eps);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_vqw2v_conv0_apply(const float* wave, long long ld_wave, const float* w, const float* stats, const float* gamma, const float* beta,
                                     float* out, int B, int C, long long Tin, long long Tout, int ksize, int stride, int logc, void* stream) {
    if (const int rc = conv0_check(B, C, Tin, Tout, ksize, stride, ld_wave)) return rc;
    conv0_apply_launch(wave, ld_wave, w, Conv0PerRowRelu{reinterpret_cast<const float2*>(stats), logc}, gamma, beta, out, B, C, Tout, ksize, stride,
                       (hipStream_t)stream);
    ALM_LAUNCH_CHECK();
    return 0;
}
