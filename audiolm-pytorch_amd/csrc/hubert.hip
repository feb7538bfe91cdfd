// HuBERT-base feature model (fairseq hubert.py / wav2vec2.py, used by the reference's hubert_kmeans.py:37-121) on gfx950, fp32 throughout:
// the output is an argmin over float distances, so every matrix product runs on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32).
// All activations are [B][C][T] (time fastest), the codec's layout, so alm_bct_to_btc / alm_rvq_encode serve unchanged.
//
//   conv0 stats    : layer 0 (Cin = 1, k = 10, stride 5) is 10 MACs per output; its per-(row, channel) GroupNorm statistics over time are taken
//                    WITHOUT storing the activation: stage 1 (conv0_stats.hpp, shared with vq_wav2vec.hip) = one thread per channel over a chunk of
//                    1024 outputs, two-level sums shifted by the mean of the chunk's first 32 outputs (a DC-heavy wave does not cancel); stage 2 = one
//                    thread per (row, channel) merging the chunks in index order (Chan's update, fp64).  No atomics: bitwise deterministic.
//   conv0 apply    : recomputes the conv (same fma chain), normalises, GELU, stores [B][C][T0] once (conv0_stats.hpp, the functor below).
//   layernorm      : nn.LayerNorm over channels, 32 channel slices per time step (alm_layernorm_bct's one thread per t starves at n <= 1499).
//   conv1d_valid (the convs after layer 0, every Linear, the positional conv) and mha_attn (the attention) are the shared fp32 kernels of
//   dense_f32.hip.
#include "common.hpp"
#include "conv0_stats.hpp"

namespace {

// ---- stage 2: fixed-order merge of the chunks -> stats[b][c] = (mean, rstd) (biased variance, as nn.GroupNorm) ----
__global__ __launch_bounds__(256) void conv0_stats_merge_kernel(const float2* __restrict__ part, float2* __restrict__ stats, long long BC, long long Tout,
                                                                int chunks, float eps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    double n = 0., mean = 0., M2 = 0.;
    for (int ch = 0; ch < chunks; ++ch) {
        const float2 p = part[(size_t)i * chunks + ch];
        const double nb = (double)min((long long)C0_CHUNK, Tout - (long long)ch * C0_CHUNK);
        const double delta = (double)p.x - mean, tot = n + nb;
        mean += delta * (nb / tot);
        M2 += (double)p.y + delta * delta * (n * nb / tot);
        n = tot;
    }
    const double var = M2 / n;
    stats[i] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)eps)));
}

// conv0 apply (conv0_stats.hpp): one (mean, rstd) per (row, channel), GELU
struct Conv0PerChannelGelu {
    const float2* __restrict__ stats;
    int C;
    __device__ __forceinline__ float2 stat(int b, int c) const { return stats[(size_t)b * C + c]; }
    __device__ __forceinline__ float act(float v) const { return gelu_f(v); }
};

// ---- LayerNorm over the channel axis of [B][C][T], parallel over channels: 32 t x 32 channel slices per workgroup, two-pass (mean, then the
// centred sum of squares), slices reduced through LDS in slice order.  alm_layernorm_bct runs one thread per t over all C, which leaves this model's
// short sequences (n = 99 .. 1499 frames) on a handful of workgroups. ----
__global__ __launch_bounds__(1024) void ln_bct_split_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ out, int C, int T, float eps) {
    constexpr int NS = 32;                    // channel slices
    __shared__ float red[NS][33];
    const int tl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int t = blockIdx.x * 32 + tl, b = blockIdx.y;
    const bool ok = t < T;
    const float* xp = x + (size_t)b * C * T + t;
    float s = 0.f;
    if (ok)
        for (int c = sl; c < C; c += NS) s += xp[(size_t)c * T];
    red[sl][tl] = s;
    __syncthreads();
    float mean = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) mean += red[i][tl];
    mean /= (float)C;
    __syncthreads();
    float q = 0.f;
    if (ok)
        for (int c = sl; c < C; c += NS) {
            const float d = xp[(size_t)c * T] - mean;
            q = fmaf(d, d, q);
        }
    red[sl][tl] = q;
    __syncthreads();
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) var += red[i][tl];
    const float rstd = rsqrtf(var / (float)C + eps);
    if (!ok) return;
    float* op = out + (size_t)b * C * T + t;
    for (int c = sl; c < C; c += NS) op[(size_t)c * T] = (xp[(size_t)c * T] - mean) * rstd * gamma[c] + beta[c];
}

}  // namespace

extern "C" int alm_hubert_conv0_chunks(long long Tout) { return conv0_chunks(Tout); }

extern "C" int alm_hubert_conv0_stats(const float* wave, long long ld_wave, const float* w, float* part, float* stats, int B, int C, long long Tin,
                                      long long Tout, int ksize, int stride, float eps, void* stream) {
    if (const int rc = conv0_check(B, C, Tin, Tout, ksize, stride, ld_wave)) return rc;
    const int chunks = conv0_chunks(Tout);
    conv0_stats_launch(wave, ld_wave, w, reinterpret_cast<float2*>(part), B, C, Tin, Tout, ksize, stride, (hipStream_t)stream);
    const long long BC = (long long)B * C;
    hipLaunchKernelGGL(conv0_stats_merge_kernel, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2*>(part), reinterpret_cast<float2*>(stats), BC, Tout, chunks, eps);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_hubert_conv0_apply(const float* wave, long long ld_wave, const float* w, const float* stats, const float* gamma, const float* beta,
                                      float* out, int B, int C, long long Tin, long long Tout, int ksize, int stride, void* stream) {
    if (const int rc = conv0_check(B, C, Tin, Tout, ksize, stride, ld_wave)) return rc;
    conv0_apply_launch(wave, ld_wave, w, Conv0PerChannelGelu{reinterpret_cast<const float2*>(stats), C}, gamma, beta, out, B, C, Tout, ksize, stride,
                       (hipStream_t)stream);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_layernorm_bct_split(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int T, float eps, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0) return ALM_ERR_BAD_ARG;
    if (B > 65535) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ln_bct_split_kernel, dim3((T + 31) / 32, B), dim3(1024), 0, (hipStream_t)stream, x, gamma, beta, out, C, T, eps);
    ALM_LAUNCH_CHECK();
    return 0;
}
