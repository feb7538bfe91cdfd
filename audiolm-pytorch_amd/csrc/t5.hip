// T5 text encoder (transformers T5Stack as the reference's t5.py:68-110 calls it, restated in tests/t5_restated.py) on gfx950, fp32 throughout,
// inference only (the encoder is frozen: no backward).  Activations are [C][N], N = B * T: the codec's [B][C][T] with the batch folded into the
// time axis, so that a batch of short prompts fills the 64-wide time tiles of alm_conv1d_valid (ksize = 1: every bias-less Linear of the model,
// q | k | v and wi_0 | wi_1 stacked) instead of leaving most of each tile empty.  Only the gather and the attention know where a sample starts.
//
//   embed     : out[c][n] = shared[ids[n]][c], 32 x 32 tiles turned through LDS (table rows are read along c, the activation is written along n).
//               An id outside [0, vocab) is never dereferenced: zero column + the device error word, as embed_assemble_kernel.
//   rmsnorm   : T5LayerNorm, y = w x rsqrt(mean(x^2) + eps): no mean, no bias.  32 columns x 32 channel slices per workgroup, the slices summed
//               through LDS in slice order (fixed order: deterministic).  Optional key mask: exact 0.0 where mask == 0.  The final norm writes
//               [N][C] row-major (= (b, n, d_model)) through 32 x 32 LDS tiles: no transpose launch.
//   attention : mha_attn_kernel of hubert.hip (a wave owns 32 queries, K / V tiles of 32 keys through LDS, S^T = K Q^T, online softmax in-lane)
//               plus T5's terms: no 1 / sqrt(d) scale, score += bias[h][key - query + T - 1] (one head's row of the dense [H][2T - 1] table
//               sits in LDS), a key with mask 0 gets probability exactly 0, a row with every key masked gives zeros (no NaN); key tiles
//               that are padding throughout are skipped.
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

// ---- bidirectional attention, head width 64: qkv [3 H 64][N] -> out [H 64][N], sample b = columns b T .. b T + T - 1 ----
__global__ __launch_bounds__(256) void t5_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bias, const unsigned char* __restrict__ mask,
                                                      float* __restrict__ out, int H, int T, size_t N) {
    __shared__ float Ks[64][32];
    __shared__ float Vs[64][33];
    __shared__ __align__(16) unsigned char Ms[32];
    extern __shared__ float bs[];                     // this head's bias row, [2 T - 1] (+ 32 never-used floats), index key - query + T - 1
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const size_t D = (size_t)H * 64;
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const float* base = qkv + (size_t)b * T;
    const float* Q = base + (size_t)(h * 64) * N;
    const float* K = base + (D + h * 64) * N;
    const float* V = base + (2 * D + h * 64) * N;
    const unsigned char* mrow = mask ? mask + (size_t)b * T : nullptr;

    for (int i = tid; i < 2 * T - 1; i += 256) bs[i] = bias[(size_t)h * (2 * T - 1) + i];
    const int boff = T - 1 - min(q, T - 1);           // a lane past the last query reads the last query's entries: always inside the row

    float qreg[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) qreg[kk] = q < T ? Q[(size_t)(2 * kk + lh) * N + q] : 0.f;
    f32x16 o0, o1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { o0[v] = 0.f; o1[v] = 0.f; }
    float m = -INFINITY, l = 0.f;

    const int lkey = tid & 31, ld0 = tid >> 5;        // tile loads: key = lkey, d = ld0 + 8 i
    float kreg[8], vreg[8];                           // the next tile, in flight while the matrix core works on the current one
    unsigned char mreg = 0;
    auto fetch = [&](int k0) {
        const bool ok = k0 + lkey < T;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t o = (size_t)(ld0 + 8 * i) * N + k0 + lkey;
            kreg[i] = ok ? K[o] : 0.f;
            vreg[i] = ok ? V[o] : 0.f;
        }
        if (ld0 == 0) mreg = ok ? (mrow ? mrow[k0 + lkey] : 1) : 0;
    };
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += 32) {
        __syncthreads();                              // also orders the bias row before its first use
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            Ks[ld0 + 8 * i][lkey] = kreg[i];
            Vs[ld0 + 8 * i][lkey] = vreg[i];
        }
        if (ld0 == 0) Ms[lkey] = mreg;
        __syncthreads();
        if (k0 + 32 < T) fetch(k0 + 32);
        // a tile without one key that counts (the padding of a short text) changes nothing below: every weight is 0 and the rescale factor is
        // exp(0) = 1 (or 0 on an accumulator that is still 0), so leaving it out gives the same bits.  The test is uniform over the workgroup.
        const uint4 mw0 = *reinterpret_cast<const uint4*>(Ms), mw1 = *reinterpret_cast<const uint4*>(Ms + 16);
        if (!(mw0.x | mw0.y | mw0.z | mw0.w | mw1.x | mw1.y | mw1.z | mw1.w)) continue;
        f32x16 s;
#pragma unroll
        for (int v = 0; v < 16; ++v) s[v] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[2 * kk + lh][lr], qreg[kk], s, 0, 0, 0);
        // s[v] = score of key k0 + (v & 3) + 8 (v >> 2) + 4 lh against query `q` (this lane's column)
        float tmax = -INFINITY;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int kl = (v & 3) + 8 * (v >> 2) + 4 * lh;
            s[v] = Ms[kl] ? s[v] + bs[k0 + kl + boff] : -INFINITY;        // Ms is 0 past the last key: the entry used is <= 2 T - 2 (the row is allocated 32 floats longer)
            tmax = fmaxf(tmax, s[v]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);
        const float ms = mn == -INFINITY ? 0.f : mn;  // every key so far masked: exp(-inf - 0) = 0 below, no inf - inf
        const float alpha = expf(m - ms);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            s[v] = expf(s[v] - ms);
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
    const float inv = l > 0.f ? 1.f / l : 0.f;        // every key masked: zeros
    float* dst = out + (size_t)(h * 64) * N + (size_t)b * T + q;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int d = (v & 3) + 8 * (v >> 2) + 4 * lh;
        dst[(size_t)d * N] = o0[v] * inv;
        dst[(size_t)(d + 32) * N] = o1[v] * inv;
    }
}

constexpr int T5_MAX_T = 2048;                        // bias row of 2 T - 1 floats in LDS beside the K / V tiles

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

extern "C" int alm_t5_attn_fwd(const float* qkv, const float* bias, const unsigned char* mask, float* out, int B, int H, int T, int dim_head,
                               void* stream) {
    if (B <= 0 || H <= 0 || T <= 0 || !qkv || !bias || !out) return ALM_ERR_BAD_ARG;
    if (dim_head != 64 || B > 65535 || H > 65535 || T > T5_MAX_T || (long long)B * T >= (1LL << 31)) return ALM_ERR_UNSUPPORTED;
    const size_t smem = (size_t)(2 * T - 1 + 32) * sizeof(float);       // + 32: the tail tile's index k0 + kl + boff stays inside the allocation
                                                                       // even if the compiler reads before it selects
    hipLaunchKernelGGL(t5_attn_kernel, dim3((T + 127) / 128, H, B), dim3(256), smem, (hipStream_t)stream, qkv, bias, mask, out, H, T,
                       (size_t)B * (size_t)T);
    ALM_LAUNCH_CHECK();
    return 0;
}
