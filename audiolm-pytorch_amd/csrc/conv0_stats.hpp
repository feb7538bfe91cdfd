// Layer 0 of the wav2vec-family feature extractors (Cin = 1, a few taps, stride > 1) produces the largest activation of the model, so its
// GroupNorm statistics are taken WITHOUT storing it.  Shared by csrc/hubert.hip (GroupNorm(C, C): one (mean, rstd) per row and channel) and
// csrc/vq_wav2vec.hip (GroupNorm(1, C): one per row): both start from the same per-(row, channel, chunk) partials and differ in how they merge them.
//
//   stage 1 (conv0_stats_kernel): one thread per channel over a chunk of C0_CHUNK outputs, two-level sums shifted by the mean of the chunk's first 32
//   outputs (a DC-heavy wave does not cancel) -> part[b][c][chunk] = (mean, M2) of the chunk.  No atomics: bitwise deterministic.
//   apply (conv0_apply_kernel<Epi>): recomputes the conv (the same fma chain), normalises with the model's statistics and activation, stores once.
#pragma once
#include "common.hpp"

namespace {

constexpr int C0_CHUNK = 1024;        // conv0 outputs per statistics chunk
constexpr int C0_MAXK = 16;
constexpr int C0_MAX_LDS = 12288;     // floats of one chunk's input window

// ---- conv0 statistics, stage 1: part[b][c][chunk] = (mean, M2) of the chunk ----
__global__ __launch_bounds__(256) void conv0_stats_kernel(const float* __restrict__ wave, long long ldw, const float* __restrict__ w,
                                                          float2* __restrict__ part, int C, long long Tin, long long Tout, int ksize, int stride,
                                                          int chunks) {
    extern __shared__ float xs[];
    const int chunk = blockIdx.x, b = blockIdx.z;
    const int c = blockIdx.y * 256 + threadIdx.x;
    const long long t0 = (long long)chunk * C0_CHUNK;
    const int n = (int)min((long long)C0_CHUNK, Tout - t0);
    const int span = (n - 1) * stride + ksize;
    const float* src = wave + (size_t)b * ldw + t0 * stride;
    for (int i = threadIdx.x; i < span; i += 256) xs[i] = src[i];           // t0 * stride + span <= (Tout - 1) * stride + ksize <= Tin
    __syncthreads();
    if (c >= C) return;
    float wk[C0_MAXK];
#pragma unroll
    for (int k = 0; k < C0_MAXK; ++k) wk[k] = k < ksize ? w[(size_t)c * ksize + k] : 0.f;
    auto conv = [&](int t) {
        const float* xp = xs + t * stride;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < C0_MAXK; ++k)
            if (k < ksize) v = fmaf(wk[k], xp[k], v);
        return v;
    };
    // shift = mean of the chunk's first 32 outputs: within a standard error of the chunk mean, so s2 - s1^2 / n below does not cancel
    float shift = 0.f;
    const int nh = min(32, n);
    for (int t = 0; t < nh; ++t) shift += conv(t);
    shift /= (float)nh;
    // two-level sums (32 outputs, then the chunk): the fp32 summation error is (32 + 32) u relative instead of 1024 u
    float s1 = 0.f, s2 = 0.f;
    for (int tb = 0; tb < n; tb += 32) {
        float a1 = 0.f, a2 = 0.f;
        const int te = min(tb + 32, n);
        for (int t = tb; t < te; ++t) {
            const float d = conv(t) - shift;
            a1 += d;
            a2 = fmaf(d, d, a2);
        }
        s1 += a1;
        s2 += a2;
    }
    const float mean_d = s1 / (float)n;
    part[((size_t)b * C + c) * chunks + chunk] = make_float2(shift + mean_d, fmaxf(s2 - s1 * mean_d, 0.f));
}

inline int conv0_chunks(long long Tout) { return Tout <= 0 ? 0 : (int)((Tout + C0_CHUNK - 1) / C0_CHUNK); }

inline int conv0_check(int B, int C, long long Tin, long long Tout, int ksize, int stride, long long ld_wave) {
    if (B <= 0 || C <= 0 || Tout <= 0 || ksize <= 0 || stride <= 0 || ld_wave < Tin) return ALM_ERR_BAD_ARG;
    if (Tin < ksize || Tout != (Tin - ksize) / stride + 1) return ALM_ERR_BAD_ARG;
    if (ksize > C0_MAXK || (long long)(C0_CHUNK - 1) * stride + ksize > C0_MAX_LDS || B > 65535) return ALM_ERR_UNSUPPORTED;
    if ((Tout + 255) / 256 > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    return 0;
}

// launches stage 1 for a checked shape (conv0_check): part = [B][C][conv0_chunks(Tout)] float2
inline void conv0_stats_launch(const float* wave, long long ld_wave, const float* w, float2* part, int B, int C, long long Tin, long long Tout, int ksize,
                               int stride, hipStream_t stream) {
    const int chunks = conv0_chunks(Tout);
    const size_t smem = (size_t)((C0_CHUNK - 1) * stride + ksize) * sizeof(float);
    hipLaunchKernelGGL(conv0_stats_kernel, dim3(chunks, (C + 255) / 256, B), dim3(256), smem, stream, wave, ld_wave, w, part, C, Tin, Tout, ksize,
                       stride, chunks);
}

// ---- conv0 apply: out[b][c][t] = act(((conv - mean) * rstd) * gamma + beta); thread = one t, 64 channels per workgroup.  The conv is the fma chain of
// stage 1.  Epi supplies what the two models differ in: stat(b, c) -> (mean, rstd) of that row and channel, act(v) -> the activation. ----
constexpr int C0_CG = 64;
template <class Epi>
__global__ __launch_bounds__(256) void conv0_apply_kernel(const float* __restrict__ wave, long long ldw, const float* __restrict__ w, const Epi epi,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out, int C,
                                                          long long Tout, int ksize, int stride) {
    __shared__ float ws[C0_CG][C0_MAXK];
    __shared__ float4 aff[C0_CG];            // mean, rstd, gamma, beta
    const int b = blockIdx.z, c0 = blockIdx.y * C0_CG;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < C0_CG * C0_MAXK; i += 256) {
        const int c = c0 + i / C0_MAXK, k = i % C0_MAXK;
        ws[i / C0_MAXK][k] = (c < C && k < ksize) ? w[(size_t)c * ksize + k] : 0.f;
    }
    if (threadIdx.x < C0_CG) {
        const int c = c0 + threadIdx.x;
        if (c < C) {
            const float2 s = epi.stat(b, c);
            aff[threadIdx.x] = make_float4(s.x, s.y, gamma[c], beta[c]);
        } else {
            aff[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __syncthreads();
    if (t >= Tout) return;
    float xv[C0_MAXK];
    const float* src = wave + (size_t)b * ldw + t * stride;
#pragma unroll
    for (int k = 0; k < C0_MAXK; ++k) xv[k] = k < ksize ? src[k] : 0.f;
    const int nc = min(C0_CG, C - c0);
    float* dst = out + ((size_t)b * C + c0) * Tout + t;
    for (int cl = 0; cl < nc; ++cl) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < C0_MAXK; ++k)
            if (k < ksize) v = fmaf(ws[cl][k], xv[k], v);
        const float4 a = aff[cl];
        dst[(size_t)cl * Tout] = epi.act((v - a.x) * a.y * a.z + a.w);
    }
}

// for a checked shape (conv0_check)
template <class Epi>
inline void conv0_apply_launch(const float* wave, long long ld_wave, const float* w, const Epi& epi, const float* gamma, const float* beta, float* out,
                               int B, int C, long long Tout, int ksize, int stride, hipStream_t stream) {
    hipLaunchKernelGGL(conv0_apply_kernel<Epi>, dim3((unsigned)((Tout + 255) / 256), (C + C0_CG - 1) / C0_CG, B), dim3(256), 0, stream, wave, ld_wave, w,
                       epi, gamma, beta, out, C, Tout, ksize, stride);
}

}  // namespace
