// HuBERT-base feature model (fairseq hubert.py / wav2vec2.py, used by the reference's hubert_kmeans.py:37-121) on gfx950, fp32 throughout:
// the output is an argmin over float distances, so every matrix product runs on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32).
// All activations are [B][C][T] (time fastest), the codec's layout, so alm_bct_to_btc / alm_rvq_encode serve unchanged.
//
//   conv0 stats    : layer 0 (Cin = 1, k = 10, stride 5) is 10 MACs per output; its per-(row, channel) GroupNorm statistics over time are taken
//                    WITHOUT storing the activation: stage 1 = one thread per channel over a chunk of 1024 outputs, two-level sums shifted by the mean of
//                    the chunk's first 32 outputs (a DC-heavy wave does not cancel); stage 2 = one thread per (row, channel) merging the chunks in index order
//                    (Chan's update, fp64).  No atomics: bitwise deterministic.
//   conv0 apply    : recomputes the conv (same fma chain), normalises, GELU, stores [B][C][T0] once.
//   layernorm      : nn.LayerNorm over channels, 32 channel slices per time step (alm_layernorm_bct's one thread per t starves at n <= 1499).
//   conv1d_valid (the convs after layer 0, every Linear, the positional conv) and mha_attn (the attention) are the shared fp32 kernels of
//   dense_f32.hip.
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

// ---- conv0 apply: out[b][c][t] = gelu(((conv - mean) * rstd) * gamma + beta); thread = one t, 64 channels per workgroup ----
constexpr int C0_CG = 64;
__global__ __launch_bounds__(256) void conv0_apply_kernel(const float* __restrict__ wave, long long ldw, const float* __restrict__ w,
                                                          const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ out, int C, long long Tout, int ksize,
                                                          int stride) {
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
            const float2 s = stats[(size_t)b * C + c];
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
        dst[(size_t)cl * Tout] = gelu_f((v - a.x) * a.y * a.z + a.w);
    }
}

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

extern "C" int alm_hubert_conv0_chunks(long long Tout) { return Tout <= 0 ? 0 : (int)((Tout + C0_CHUNK - 1) / C0_CHUNK); }

static int conv0_check(int B, int C, long long Tin, long long Tout, int ksize, int stride, long long ld_wave) {
    if (B <= 0 || C <= 0 || Tout <= 0 || ksize <= 0 || stride <= 0 || ld_wave < Tin) return ALM_ERR_BAD_ARG;
    if (Tin < ksize || Tout != (Tin - ksize) / stride + 1) return ALM_ERR_BAD_ARG;
    if (ksize > C0_MAXK || (long long)(C0_CHUNK - 1) * stride + ksize > C0_MAX_LDS || B > 65535) return ALM_ERR_UNSUPPORTED;
    if ((Tout + 255) / 256 > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    return 0;
}

extern "C" int alm_hubert_conv0_stats(const float* wave, long long ld_wave, const float* w, float* part, float* stats, int B, int C, long long Tin,
                                      long long Tout, int ksize, int stride, float eps, void* stream) {
    if (const int rc = conv0_check(B, C, Tin, Tout, ksize, stride, ld_wave)) return rc;
    const int chunks = alm_hubert_conv0_chunks(Tout);
    const size_t smem = (size_t)((C0_CHUNK - 1) * stride + ksize) * sizeof(float);
    hipLaunchKernelGGL(conv0_stats_kernel, dim3(chunks, (C + 255) / 256, B), dim3(256), smem, (hipStream_t)stream, wave, ld_wave, w,
                       reinterpret_cast<float2*>(part), C, Tin, Tout, ksize, stride, chunks);
    const long long BC = (long long)B * C;
    hipLaunchKernelGGL(conv0_stats_merge_kernel, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2*>(part), reinterpret_cast<float2*>(stats), BC, Tout, chunks, eps);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_hubert_conv0_apply(const float* wave, long long ld_wave, const float* w, const float* stats, const float* gamma, const float* beta,
                                      float* out, int B, int C, long long Tin, long long Tout, int ksize, int stride, void* stream) {
    if (const int rc = conv0_check(B, C, Tin, Tout, ksize, stride, ld_wave)) return rc;
    hipLaunchKernelGGL(conv0_apply_kernel, dim3((unsigned)((Tout + 255) / 256), (C + C0_CG - 1) / C0_CG, B), dim3(256), 0, (hipStream_t)stream, wave,
                       ld_wave, w, reinterpret_cast<const float2*>(stats), gamma, beta, out, C, Tout, ksize, stride);
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
