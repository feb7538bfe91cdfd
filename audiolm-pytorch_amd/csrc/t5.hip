// T5 text encoder (transformers T5Stack as the reference's t5.py:68-110 calls it, restated in tests/t5_restated.py) on gfx950, fp32 throughout,
// inference only (the encoder is frozen: no backward).  Activations are [C][N], N = B * T: the codec's [B][C][T] with the batch folded into the
// time axis, so that a batch of short prompts fills the 64-wide time tiles of alm_conv1d_valid (dense_f32.hip; ksize = 1: every bias-less Linear of the model,
// q | k | v and wi_0 | wi_1 stacked) instead of leaving most of each tile empty.  Only the gather and the attention know where a sample starts.
//
//   embed     : out[c][n] = shared[ids[n]][c], 32 x 32 tiles turned through LDS (table rows are read along c, the activation is written along n).
//               An id outside [0, vocab) is never dereferenced: zero column + the device error word, as embed_assemble_kernel.
//   rmsnorm   : T5LayerNorm, y = w x rsqrt(mean(x^2) + eps): no mean, no bias.  32 columns x 32 channel slices per workgroup, the slices summed
//               through LDS in slice order (fixed order: deterministic).  Optional key mask: exact 0.0 where mask == 0.  The final norm writes
//               [N][C] row-major (= (b, n, d_model)) through 32 x 32 LDS tiles: no transpose launch.
//   attention : mha_f32_kernel<BIASED = true> of dense_f32.hip (alm_t5_attn_fwd): no 1 / sqrt(d) scale, score += bias[h][key - query + T - 1],
//               a key with mask 0 gets probability exactly 0, a row with every key masked gives zeros.
//   gate      : gelu_new(wi_0 x) * (wi_1 x) over the stacked GEMM output (v1.1 models), or relu(wi x) (the original t5-*).
#include "common.hpp"

namespace {

// transformers NewGELUActivation: 0.5 u (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3)))
__device__ __forceinline__ float gelu_new(float u) { return 0.5f * u * (1.f + tanhf(0.79788456080286535588f * (u + 0.044715f * u * u * u))); }

// ---- embedding gather: ids int64 [N], table [vocab][D] -> out [D][N] ----
__global__ __launch_bounds__(256) void t5_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ table, float* __restrict__ out, int N,
                                                       int D, long long vocab, int* __restrict__ err) {
    __shared__ float tile[32][33];            // [token][channel]
    const int tl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + sl + 8 * i, c = c0 + tl;
        float v = 0.f;
        if (n < N) {
            const long long id = ids[n];
            const bool ok = id >= 0 && id < vocab;
            if (ok && c < D) v = table[(size_t)id * D + c];
            if (!ok && err && tl == 0 && blockIdx.y == 0) *err = 1;
        }
        tile[sl + 8 * i][tl] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + sl + 8 * i, n = n0 + tl;
        if (c < D && n < N) out[(size_t)c * N + n] = tile[tl][sl + 8 * i];
    }
}

// ---- T5LayerNorm over the channel axis of [C][N]; TR: out is [N][C] ----
template <bool TR>
__global__ __launch_bounds__(1024) void t5_rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w, const unsigned char* __restrict__ mask,
                                                          float* __restrict__ out, int C, int N, float eps) {
    constexpr int NS = 32;                    // channel slices
    __shared__ float red[NS][33];
    __shared__ float rs[32];
    const int tl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int n0 = blockIdx.x * 32, n = n0 + tl;
    const bool ok = n < N;
    const float* xp = x + n;
    float q = 0.f;
    if (ok)
        for (int c = sl; c < C; c += NS) {
            const float v = xp[(size_t)c * N];
            q = fmaf(v, v, q);
        }
    red[sl][tl] = q;
    __syncthreads();
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) ss += red[i][tl];
    const float rstd = rsqrtf(ss / (float)C + eps);
    const bool zero = ok && mask && !mask[n];                   // written as +0.0, never as a product (x may hold anything there)
    if (!TR) {
        if (!ok) return;
        float* op = out + n;
        for (int c = sl; c < C; c += NS) op[(size_t)c * N] = zero ? 0.f : w[c] * (xp[(size_t)c * N] * rstd);
    } else {
        if (sl == 0) rs[tl] = zero ? -1.f : rstd;               // rstd > 0 always: -1 marks a masked column
        // red is free again after this barrier: it becomes the [channel][column] tile
        for (int c0 = 0; c0 < C; c0 += 32) {
            __syncthreads();
            red[sl][tl] = (ok && c0 + sl < C) ? xp[(size_t)(c0 + sl) * N] : 0.f;
            __syncthreads();
            const int no = n0 + sl, c = c0 + tl;
            if (no < N && c < C) {
                const float r = rs[sl];
                out[(size_t)no * C + c] = r < 0.f ? 0.f : w[c] * (red[tl][sl] * r);
            }
        }
    }
}

// ---- FFN gate: x [2F][N] -> out [F][N] = gelu_new(x[f]) * x[F + f], or x [F][N] -> relu ----
template <bool GATED>
__global__ __launch_bounds__(256) void t5_gate_kernel(const float* __restrict__ x, float* __restrict__ out, size_t FN) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < FN; i += stride) {
        if (GATED)
            out[i] = gelu_new(x[i]) * x[FN + i];
        else
            out[i] = fmaxf(x[i], 0.f);
    }
}

}  // namespace

extern "C" int alm_t5_embed(const long long* ids, const float* table, float* out, int N, int D, long long vocab, int* err_flag, void* stream) {
    if (N <= 0 || D <= 0 || vocab <= 0 || !ids || !table || !out) return ALM_ERR_BAD_ARG;
    if ((D + 31) / 32 > 65535) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(t5_embed_kernel, dim3((N + 31) / 32, (D + 31) / 32), dim3(256), 0, (hipStream_t)stream, ids, table, out, N, D, vocab, err_flag);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_t5_rmsnorm(const float* x, const float* w, const unsigned char* mask, float* out, int C, int N, float eps, int transpose_out,
                              void* stream) {
    if (C <= 0 || N <= 0 || !x || !w || !out || x == out) return ALM_ERR_BAD_ARG;
    const dim3 grid((N + 31) / 32), block(1024);
    if (transpose_out)
        hipLaunchKernelGGL(t5_rmsnorm_kernel<true>, grid, block, 0, (hipStream_t)stream, x, w, mask, out, C, N, eps);
    else
        hipLaunchKernelGGL(t5_rmsnorm_kernel<false>, grid, block, 0, (hipStream_t)stream, x, w, mask, out, C, N, eps);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_t5_gate(const float* x, float* out, long long F, long long N, int gated, void* stream) {
    if (F <= 0 || N <= 0 || !x || !out) return ALM_ERR_BAD_ARG;
    if (F > (1LL << 40) / N) return ALM_ERR_UNSUPPORTED;
    const size_t FN = (size_t)F * (size_t)N;
    const unsigned blocks = (unsigned)((FN + 1023) / 1024 < 65536 ? (FN + 1023) / 1024 : 65536);
    if (gated)
        hipLaunchKernelGGL(t5_gate_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, out, FN);
    else
        hipLaunchKernelGGL(t5_gate_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, out, FN);
    ALM_LAUNCH_CHECK();
    return 0;
}
