// HuBERT-base feature model (fairseq hubert.py / wav2vec2.py, used by the reference's hubert_kmeans.py:37-121) on gfx950, fp32 throughout:
// the output is an argmin over float distances, so every matrix product runs on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32).
// All activations are [B][C][T] (time fastest), the codec's layout, so alm_bct_to_btc / alm_rvq_encode serve unchanged.
//
//   conv0 stats    : layer 0 (Cin = 1, k = 10, stride 5) is 10 MACs per output; its per-(row, channel) GroupNorm statistics over time are taken
//                    WITHOUT storing the activation: stage 1 = one thread per channel over a chunk of 1024 outputs, two-level sums shifted by the mean of
//                    the chunk's first 32 outputs (a DC-heavy wave does not cancel); stage 2 = one thread per (row, channel) merging the chunks in index order
//                    (Chan's update, fp64).  No atomics: bitwise deterministic.
//   conv0 apply    : recomputes the conv (same fma chain), normalises, GELU, stores [B][C][T0] once.
//   conv1d_valid   : implicit GEMM of an unpadded / zero-padded, strided, grouped conv1d: 64 (Cout) x 64 (T) tile per workgroup of 4 waves, each
//                    wave a 32 x 32 block; the reduction index r = ci * ksize + k runs in chunks of 32 through LDS (weights [64][32], im2col'd
//                    input [32][64]); the next chunk's global loads are in flight while the matrix core works on the current one.
//                    Epilogue: + bias, erf-GELU, + residual.  k = 1 is the Linear layers; groups = 16, k = 128, pad = 64 the positional conv.
//   layernorm      : nn.LayerNorm over channels, 32 channel slices per time step (alm_layernorm_bct's one thread per t starves at n <= 1499).
//   mha_attn       : bidirectional multi-head attention, head width 64, flash style: a wave owns 32 queries (Q^T in registers, pre-scaled as
//                    fairseq scales q), walks the keys 32 at a time from LDS, S^T = K Q^T puts one query per lane so that the online-softmax
//                    row statistics are in-lane plus ONE exchange with lane ^ 32; P^T feeds O^T = V^T P^T straight from the accumulator
//                    registers (the key order of that sum is the accumulator's row order on both operands).
#include "common.hpp"

namespace {

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

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
        dst[(size_t)cl * Tout] = gelu_erf((v - a.x) * a.y * a.z + a.w);
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

// ---- general conv1d as an implicit GEMM on the fp32 matrix core ----
struct ConvArgs {
    const float* x; const float* w; const float* bias; const float* res; float* out;
    int Cin, Cout, Tin, Tout, ksize, stride, pad, groups, gelu;
};
constexpr int CV_RK = 32;

template <int KS>
__global__ __launch_bounds__(256) void conv_valid_kernel(ConvArgs a) {
    __shared__ float As[64][CV_RK + 1];
    __shared__ float Bs[CV_RK][64];
    const int ks = KS ? KS : a.ksize;
    const int Cig = a.Cin / a.groups, Cog = a.Cout / a.groups;
    const int R = Cig * ks;
    const int tiles_co = (Cog + 63) / 64;
    const int g = blockIdx.y / tiles_co, co0 = (blockIdx.y % tiles_co) * 64;
    const int t0 = blockIdx.x * 64, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const float* xb = a.x + ((size_t)b * a.Cin + (size_t)g * Cig) * a.Tin;
    const float* wg = a.w + (size_t)g * Cog * R;

    const int ar = tid & 31, aco = tid >> 5;          // A: r = ar, co = aco + 8 i
    const int bt = tid & 63, br = tid >> 6;           // B: t = bt, r = br + 4 i
    const bool tok = t0 + bt < a.Tout;
    const int tbase = (t0 + bt) * a.stride - a.pad;
    float areg[8], breg[8];
    auto load = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int co = co0 + aco + 8 * i, r = r0 + ar;
            areg[i] = (co < Cog && r < R) ? wg[(size_t)co * R + r] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rr = r0 + br + 4 * i;
            const int ci = rr / ks, k = rr - ci * ks;
            const int ti = tbase + k;
            breg[i] = (tok && rr < R && ti >= 0 && ti < a.Tin) ? xb[(size_t)ci * a.Tin + ti] : 0.f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) As[aco + 8 * i][ar] = areg[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) Bs[br + 4 * i][bt] = breg[i];
    };
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    load(0);
    stage();
    __syncthreads();
    for (int r0 = 0; r0 < R; r0 += CV_RK) {
        const bool more = r0 + CV_RK < R;
        if (more) load(r0 + CV_RK);
#pragma unroll
        for (int kk = 0; kk < CV_RK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[wm * 32 + lr][2 * kk + lh], Bs[2 * kk + lh][wn * 32 + lr], acc, 0, 0, 0);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    const int t = t0 + wn * 32 + lr;
    if (t >= a.Tout) return;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int co = co0 + wm * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
        if (co < Cog) {
            const int cg = g * Cog + co;
            float y = acc[v];
            if (a.bias) y += a.bias[cg];
            if (a.gelu) y = gelu_erf(y);
            const size_t o = ((size_t)b * a.Cout + cg) * a.Tout + t;
            if (a.res) y += a.res[o];
            a.out[o] = y;
        }
    }
}

// ---- bidirectional multi-head attention, head width 64: qkv [B][3 H 64][T] -> out [B][H 64][T] ----
__global__ __launch_bounds__(256) void mha_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int H, int T, float scale) {
    __shared__ float Ks[64][32];
    __shared__ float Vs[64][33];
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int D = H * 64;
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const float* base = qkv + (size_t)b * 3 * D * T;
    const float* Q = base + (size_t)(h * 64) * T;
    const float* K = base + (size_t)(D + h * 64) * T;
    const float* V = base + (size_t)(2 * D + h * 64) * T;

    float qreg[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) qreg[kk] = q < T ? Q[(size_t)(2 * kk + lh) * T + q] * scale : 0.f;
    f32x16 o0, o1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { o0[v] = 0.f; o1[v] = 0.f; }
    float m = -INFINITY, l = 0.f;

    const int lkey = tid & 31, ld0 = tid >> 5;        // tile loads: key = lkey, d = ld0 + 8 i
    float kreg[8], vreg[8];                           // the next tile, in flight while the matrix core works on the current one
    auto fetch = [&](int k0) {
        const bool ok = k0 + lkey < T;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t o = (size_t)(ld0 + 8 * i) * T + k0 + lkey;
            kreg[i] = ok ? K[o] : 0.f;
            vreg[i] = ok ? V[o] : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            Ks[ld0 + 8 * i][lkey] = kreg[i];
            Vs[ld0 + 8 * i][lkey] = vreg[i];
        }
        __syncthreads();
        if (k0 + 32 < T) fetch(k0 + 32);
        f32x16 s;
#pragma unroll
        for (int v = 0; v < 16; ++v) s[v] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[2 * kk + lh][lr], qreg[kk], s, 0, 0, 0);
        // s[v] = score of key k0 + (v & 3) + 8 (v >> 2) + 4 lh against query `q` (this lane's column)
        float tmax = -INFINITY;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int key = k0 + (v & 3) + 8 * (v >> 2) + 4 * lh;
            if (key >= T) s[v] = -INFINITY;
            tmax = fmaxf(tmax, s[v]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);              // finite: key k0 < T belongs to this tile
        const float alpha = expf(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            s[v] = expf(s[v] - mn);
            ps += s[v];
        }
        l = fmaf(l, alpha, ps);
#pragma unroll
        for (int v = 0; v < 16; ++v) { o0[v] *= alpha; o1[v] *= alpha; }
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int key = (st & 3) + 8 * (st >> 2) + 4 * lh;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[lr][key], s[st], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[32 + lr][key], s[st], o1, 0, 0, 0);
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (q >= T) return;
    const float inv = 1.f / l;
    float* dst = out + ((size_t)b * D + h * 64) * T + q;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int d = (v & 3) + 8 * (v >> 2) + 4 * lh;
        dst[(size_t)d * T] = o0[v] * inv;
        dst[(size_t)(d + 32) * T] = o1[v] * inv;
    }
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

extern "C" int alm_conv1d_valid(const float* x, const float* w, const float* bias, const float* residual, float* out, int B, int Cin, int Cout,
                                int Tin, int Tout, int ksize, int stride, int pad, int groups, int gelu, void* stream) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Tin <= 0 || Tout <= 0 || ksize <= 0 || stride <= 0 || pad < 0 || groups <= 0) return ALM_ERR_BAD_ARG;
    if (Cin % groups || Cout % groups) return ALM_ERR_BAD_ARG;
    const long long full = ((long long)Tin + 2LL * pad - ksize) / stride + 1;
    if ((long long)Tin + 2LL * pad < ksize || Tout > full) return ALM_ERR_BAD_ARG;          // Tout < full drops trailing outputs (SamePad)
    const long long tiles_y = (long long)((Cout / groups + 63) / 64) * groups;
    // in-row indices are 32-bit: (Tout + 63) * stride and (Cin / groups) * ksize must fit; rows and batches are offset in 64 bits
    if (((long long)Tout + 64) * stride + ksize >= (1LL << 31) || (long long)(Cin / groups) * ksize >= (1LL << 31) - 64 || tiles_y > 65535 || B > 65535)
        return ALM_ERR_UNSUPPORTED;
    ConvArgs a{x, w, bias, residual, out, Cin, Cout, Tin, Tout, ksize, stride, pad, groups, gelu};
    const dim3 grid((Tout + 63) / 64, (unsigned)tiles_y, B), block(256);
    switch (ksize) {
        case 1: hipLaunchKernelGGL(conv_valid_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(conv_valid_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(conv_valid_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
        case 128: hipLaunchKernelGGL(conv_valid_kernel<128>, grid, block, 0, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(conv_valid_kernel<0>, grid, block, 0, (hipStream_t)stream, a); break;
    }
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_mha_attn_fwd(const float* qkv, float* out, int B, int H, int T, int dim_head, float scale, void* stream) {
    if (B <= 0 || H <= 0 || T <= 0) return ALM_ERR_BAD_ARG;
    if (dim_head != 64 || B > 65535 || H > 65535) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mha_attn_kernel, dim3((T + 127) / 128, H, B), dim3(256), 0, (hipStream_t)stream, qkv, out, H, T, scale);
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
