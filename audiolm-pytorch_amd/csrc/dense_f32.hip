// The fp32 GEMM and attention that the frozen inference models share (HuBERT: hubert.hip, the T5 text encoder: t5.hip, EnCodec's LSTM projection:
// encodec.py), on gfx950.  Every matrix product runs on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32): HuBERT's output is an argmin over float
// distances, and the three models are checked against fp64 restatements.
//
//   conv1d_valid   : implicit GEMM of an unpadded / zero-padded, strided, grouped conv1d over [B][C][T]: 64 (Cout) x 64 (T) tile per workgroup of
//                    4 waves, each wave a 32 x 32 block; the reduction index r = ci * ksize + k runs in chunks of 32 through LDS (weights [64][32],
//                    im2col'd input [32][64]); the next chunk's global loads are in flight while the matrix core works on the current one.
//                    Epilogue: + bias, erf-GELU, + residual.  k = 1 is every Linear layer (T5 calls it with B = 1 and the batch folded into T);
//                    groups = 16, k = 128, pad = 64 is HuBERT's positional conv.
//   mha_f32        : bidirectional multi-head attention, head width 64, flash style: a wave owns 32 queries (Q^T in registers), walks the keys
//                    32 at a time from LDS, S^T = K Q^T puts one query per lane so that the online-softmax row statistics are in-lane plus ONE
//                    exchange with lane ^ 32; P^T feeds O^T = V^T P^T straight from the accumulator registers (the key order of that sum is the
//                    accumulator's row order on both operands).  Rows of q | k | v are `pitch` floats apart and sample b starts `in_batch` floats
//                    into a row, so one kernel reads HuBERT's [B][3 H 64][T] (pitch T, in_batch 3 H 64 T, out_batch H 64 T) and T5's
//                    [3 H 64][B T] (pitch B T, in_batch = out_batch = T).
//                    BIASED = false (alm_mha_attn_fwd): Q is pre-scaled by `scale`, as fairseq scales q.
//                    BIASED = true (alm_t5_attn_fwd): no scale; score += bias[h][key - query + T - 1] (one head's row of the dense [H][2T - 1]
//                    table sits in LDS); a key with mask 0 gets probability exactly 0, a row with every key masked gives zeros (no NaN); key
//                    tiles that are padding throughout are skipped.
#include "common.hpp"

namespace {

// ---- general conv1d as an implicit GEMM on the fp32 matrix core ----
struct ConvValidArgs {
    const float* x; const float* w; const float* bias; const float* res; float* out;
    int Cin, Cout, Tin, Tout, ksize, stride, pad, groups, gelu;
};
constexpr int CV_RK = 32;

template <int KS>
__global__ __launch_bounds__(256) void conv_valid_kernel(ConvValidArgs a) {
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
            if (a.gelu) y = gelu_f(y);
            const size_t o = ((size_t)b * a.Cout + cg) * a.Tout + t;
            if (a.res) y += a.res[o];
            a.out[o] = y;
        }
    }
}

// ---- bidirectional multi-head attention, head width 64: q | k | v rows [3 H 64] x pitch -> out rows [H 64] x pitch ----
struct MhaF32Args {
    const float* qkv; const float* bias; const unsigned char* mask; float* out;
    int H, T;
    size_t pitch, in_batch, out_batch;                // floats between rows; floats from sample b to b + 1 in qkv and in out
    float scale;
};

template <bool BIASED>                                // relative-position bias row + key-mask bytes
__global__ __launch_bounds__(256) void mha_f32_kernel(MhaF32Args a) {
    __shared__ float Ks[64][32];
    __shared__ float Vs[64][33];
    __shared__ __align__(16) unsigned char Ms[32];    // BIASED only
    extern __shared__ float bs[];                     // BIASED only: this head's bias row, [2 T - 1] (+ 32 never-used floats), index key - query + T - 1
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int T = a.T;
    const size_t D = (size_t)a.H * 64, P = a.pitch;
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const float* base = a.qkv + (size_t)b * a.in_batch;
    const float* Q = base + (size_t)(h * 64) * P;
    const float* K = base + (D + h * 64) * P;
    const float* V = base + (2 * D + h * 64) * P;
    const unsigned char* mrow = nullptr;
    int boff = 0;
    if constexpr (BIASED) {
        if (a.mask) mrow = a.mask + (size_t)b * T;
        for (int i = tid; i < 2 * T - 1; i += 256) bs[i] = a.bias[(size_t)h * (2 * T - 1) + i];
        boff = T - 1 - min(q, T - 1);                 // a lane past the last query reads the last query's entries: always inside the row
    }

    float qreg[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        if constexpr (BIASED)
            qreg[kk] = q < T ? Q[(size_t)(2 * kk + lh) * P + q] : 0.f;
        else
            qreg[kk] = q < T ? Q[(size_t)(2 * kk + lh) * P + q] * a.scale : 0.f;
    }
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
            const size_t o = (size_t)(ld0 + 8 * i) * P + k0 + lkey;
            kreg[i] = ok ? K[o] : 0.f;
            vreg[i] = ok ? V[o] : 0.f;
        }
        if constexpr (BIASED)
            if (ld0 == 0) mreg = ok ? (mrow ? mrow[k0 + lkey] : 1) : 0;
    };
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += 32) {
        __syncthreads();                              // BIASED: also orders the bias row before its first use
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            Ks[ld0 + 8 * i][lkey] = kreg[i];
            Vs[ld0 + 8 * i][lkey] = vreg[i];
        }
        if constexpr (BIASED)
            if (ld0 == 0) Ms[lkey] = mreg;
        __syncthreads();
        if (k0 + 32 < T) fetch(k0 + 32);
        if constexpr (BIASED) {
            // a tile without one key that counts (the padding of a short text) changes nothing below: every weight is 0 and the rescale factor is
            // exp(0) = 1 (or 0 on an accumulator that is still 0), so leaving it out gives the same bits.  The test is uniform over the workgroup.
            const uint4 mw0 = *reinterpret_cast<const uint4*>(Ms), mw1 = *reinterpret_cast<const uint4*>(Ms + 16);
            if (!(mw0.x | mw0.y | mw0.z | mw0.w | mw1.x | mw1.y | mw1.z | mw1.w)) continue;
        }
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
            if constexpr (BIASED)
                s[v] = Ms[kl] ? s[v] + bs[k0 + kl + boff] : -INFINITY;        // Ms is 0 past the last key: the entry used is <= 2 T - 2 (the row is allocated 32 floats longer)
            else if (k0 + kl >= T)
                s[v] = -INFINITY;
            tmax = fmaxf(tmax, s[v]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);              // !BIASED: finite, key k0 < T belongs to this tile
        float ms = mn;
        if constexpr (BIASED) ms = mn == -INFINITY ? 0.f : mn;        // every key so far masked: exp(-inf - 0) = 0 below, no inf - inf
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
    float inv = 1.f / l;
    if constexpr (BIASED) inv = l > 0.f ? 1.f / l : 0.f;              // every key masked: zeros
    float* dst = a.out + (size_t)b * a.out_batch + (size_t)(h * 64) * P + q;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int d = (v & 3) + 8 * (v >> 2) + 4 * lh;
        dst[(size_t)d * P] = o0[v] * inv;
        dst[(size_t)(d + 32) * P] = o1[v] * inv;
    }
}

constexpr int T5_MAX_T = 2048;                        // bias row of 2 T - 1 floats in LDS beside the K / V tiles

}  // namespace

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
    ConvValidArgs a{x, w, bias, residual, out, Cin, Cout, Tin, Tout, ksize, stride, pad, groups, gelu};
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

// HuBERT: qkv [B][3 H 64][T] -> out [B][H 64][T]
extern "C" int alm_mha_attn_fwd(const float* qkv, float* out, int B, int H, int T, int dim_head, float scale, void* stream) {
    if (B <= 0 || H <= 0 || T <= 0) return ALM_ERR_BAD_ARG;
    if (dim_head != 64 || B > 65535 || H > 65535) return ALM_ERR_UNSUPPORTED;
    const size_t DT = (size_t)H * 64 * (size_t)T;
    MhaF32Args a{qkv, nullptr, nullptr, out, H, T, (size_t)T, 3 * DT, DT, scale};
    hipLaunchKernelGGL(mha_f32_kernel<false>, dim3((T + 127) / 128, H, B), dim3(256), 0, (hipStream_t)stream, a);
    ALM_LAUNCH_CHECK();
    return 0;
}

// T5: qkv [3 H 64][N] -> out [H 64][N], N = B T, sample b = columns b T .. b T + T - 1
extern "C" int alm_t5_attn_fwd(const float* qkv, const float* bias, const unsigned char* mask, float* out, int B, int H, int T, int dim_head,
                               void* stream) {
    if (B <= 0 || H <= 0 || T <= 0 || !qkv || !bias || !out) return ALM_ERR_BAD_ARG;
    if (dim_head != 64 || B > 65535 || H > 65535 || T > T5_MAX_T || (long long)B * T >= (1LL << 31)) return ALM_ERR_UNSUPPORTED;
    const size_t smem = (size_t)(2 * T - 1 + 32) * sizeof(float);       // + 32: the tail tile's index k0 + kl + boff stays inside the allocation
                                                                       // even if the compiler reads before it selects
    MhaF32Args a{qkv, bias, mask, out, H, T, (size_t)B * (size_t)T, (size_t)T, (size_t)T, 0.f};
    hipLaunchKernelGGL(mha_f32_kernel<true>, dim3((T + 127) / 128, H, B), dim3(256), smem, (hipStream_t)stream, a);
    ALM_LAUNCH_CHECK();
    return 0;
}
