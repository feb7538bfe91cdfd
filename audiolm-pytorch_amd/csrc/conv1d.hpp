// The causal conv1d implicit GEMM shared by csrc/codec.hip (SoundStream) and csrc/encodec.hip (EnCodec's SEANet); see codec.hip's header comment.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace {

// ELU(alpha = 1): v > 0 ? v : exp(v) - 1, branch-free.  Near zero exp(v) - 1 cancels, so |v| < 0.35 uses the degree-8 Taylor polynomial
// (truncation < 1e-9 relative); elsewhere exp2 (<= 2 ulp) minus one loses < 2 bits.  Agrees with expm1f to a few ulp.
__device__ __forceinline__ float elu1(float v) {
    const float em = __builtin_amdgcn_exp2f(v * 1.4426950408889634f) - 1.f;
    float p = 2.48015873e-5f;                                                   // 1/8!
    p = fmaf(p, v, 1.98412698e-4f);
    p = fmaf(p, v, 1.38888889e-3f);
    p = fmaf(p, v, 8.33333333e-3f);
    p = fmaf(p, v, 4.16666667e-2f);
    p = fmaf(p, v, 1.66666667e-1f);
    p = fmaf(p, v, 0.5f);
    p = fmaf(p, v, 1.f);
    p *= v;
    const float neg = v > -0.35f ? p : em;
    return v > 0.f ? v : neg;
}

struct ConvArgs {
    const float* x; const float* wp; const float* bias; const float* residual; float* out;
    int B, Cin, CinP, Cout, CoutP, Tin, Tout, ks, stride, dil, pad, elu;
    int zero_pad;       // 0: reflect left pad (CausalConv1d, soundstream.py:343); 1: zeros left of the signal (the k = 2 form of a transposed conv)
};

// grid: (ceil(Tout / 256), CoutP / (32 * NA), B); 4 waves along time, 64 output steps each
// PRE: ELU on the activation operand as it is fed to the matrix core (EnCodec's SEANet applies ELU BEFORE each conv, csrc/encodec.hip).  ELU(0) = 0 and
// a reflected sample is a sample, so this commutes with both paddings; SoundStream's convs instantiate PRE = false (the code they always were).
template <int NA, bool PRE = false>
__global__ __launch_bounds__(256, 2) void conv1d_causal_kernel(ConvArgs a) {      // (256, 2): without the occupancy hint the compiler parks copies in AGPRs (184 registers, NA = 2)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int b = blockIdx.z;
    const int co0 = blockIdx.y * 32 * NA;
    const int t0 = blockIdx.x * 256 + wave * 64;
    if (t0 >= a.Tout) return;
    const float* xb = a.x + (long long)b * a.Cin * a.Tin;

    f32x16 acc[NA][2];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    int tin[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) tin[j] = (t0 + j * 32 + lr) * a.stride - a.pad;

    // The (tap, channel-pair) contraction steps are flattened into one sequence and software-pipelined by hand: two register groups of U
    // steps, the loads of group g + 1 are issued before the MFMAs of group g.  All addressing is 32-bit buffer addressing: a per-lane byte
    // offset that only changes with the tap (reflect-padded time index) plus a wave-uniform scalar offset per step -- no 64-bit VALU
    // multiplies in the loop (they, not the loads, were what limited the first version).  Channels >= Cin meet zero-padded weights and
    // read 0 past the end of this batch element's buffer; time steps >= Tout compute garbage that is never stored.
    constexpr int U = 2;
    const int nk = a.CinP >> 1;                                    // channel pairs per tap
    const int nsteps = a.ks * nk, ng = (nsteps + U - 1) / U;
    const auto rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.Cin * a.Tin * 4, 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, a.ks * a.CinP * a.CoutP * 4, 0x00020000);
    const int wvo = (lh * a.CoutP + co0 + lr) * 4;
    int ltap = 0, lk = 0;                                          // next step to load (wave-uniform)
    int xvo[2];
    auto set_tap = [&](int tap) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int p = tin[j] + tap * a.dil;
            const bool left = p < 0;
            p = left ? -p : p;                                     // reflect (F.pad mode='reflect'): index -i -> i
            xvo[j] = (left && a.zero_pad) ? (int)0x80000000 : (lh * a.Tin + p) * 4;      // zero pad: out-of-range offset reads 0
        }
    };
    set_tap(0);
    float av[2][U][NA], bv[2][U][2];
    auto load_group = [&](auto bufc) {
        constexpr int BUF = decltype(bufc)::value;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ltap < a.ks) {
                const int wso = ((ltap * a.CinP + 2 * lk) * a.CoutP) * 4, xso = (2 * lk * a.Tin) * 4;
#pragma unroll
                for (int i = 0; i < NA; ++i) av[BUF][u][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsW, wvo + i * 128, wso, 0));
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[BUF][u][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsX, xvo[j], xso, 0));
                if (++lk == nk) {
                    lk = 0;
                    ++ltap;
                    set_tap(ltap);
                }
            } else {
#pragma unroll
                for (int i = 0; i < NA; ++i) av[BUF][u][i] = 0.f;
                bv[BUF][u][0] = bv[BUF][u][1] = 0.f;
            }
        }
    };
    auto mfma_group = [&](auto bufc) {
        constexpr int BUF = decltype(bufc)::value;
        if constexpr (PRE) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[BUF][u][j] = elu1(bv[BUF][u][j]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < NA; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[BUF][u][i], bv[BUF][u][j], acc[i][j], 0, 0, 0);
    };
    load_group(std::integral_constant<int, 0>{});
    for (int g = 0; g < ng; g += 2) {
        if (g + 1 < ng) load_group(std::integral_constant<int, 1>{});
        mfma_group(std::integral_constant<int, 0>{});
        if (g + 2 < ng) load_group(std::integral_constant<int, 0>{});
        if (g + 1 < ng) mfma_group(std::integral_constant<int, 1>{});
    }
    // D layout: column = lane & 31 (time), row = (r & 3) + 8 * (r >> 2) + 4 * lh (output channel).  Epilogue addressing is 32-bit buffer
    // addressing too: per-lane byte offset (channel half, time) + a wave-uniform row offset; rows >= Cout fall outside the buffer and are
    // dropped by the bounds check, lanes with t >= Tout get an out-of-range offset.
    const long long ob = (long long)b * a.Cout * a.Tout;
    const auto rsO = __builtin_amdgcn_make_buffer_rsrc(a.out + ob, 0, a.Cout * a.Tout * 4, 0x00020000);
    const auto rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.residual ? a.residual + ob : a.out + ob), 0, a.Cout * a.Tout * 4, 0x00020000);
    const auto rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.Cout * 4, 0x00020000);
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        float bias[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x4 bq = __builtin_amdgcn_raw_buffer_load_b128(rsB, (co0 + i * 32 + 8 * g + 4 * lh) * 4, 0, 0);      // channels >= Cout read 0
#pragma unroll
            for (int c = 0; c < 4; ++c) bias[4 * g + c] = __uint_as_float(bq[c]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t = t0 + j * 32 + lr;
            const int vb = t < a.Tout ? ((co0 + i * 32 + 4 * lh) * a.Tout + t) * 4 : (int)0x80000000;
            float v[16], rr[16];
            if (a.residual) {                                      // all 16 row loads in flight before the first use (they were issued and waited for one by one)
#pragma unroll
                for (int r = 0; r < 16; ++r) rr[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsR, vb, ((r & 3) + 8 * (r >> 2)) * a.Tout * 4, 0));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                v[r] = acc[i][j][r] + bias[r];
                if (a.elu) v[r] = elu1(v[r]);
            }
            if (a.residual) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += rr[r];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[r]), rsO, vb, ((r & 3) + 8 * (r >> 2)) * a.Tout * 4, 0);
        }
    }
}

}  // namespace
