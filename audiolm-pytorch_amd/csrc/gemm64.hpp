// The functor-parameterised 64 x 64 tile GEMM on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32), shared by csrc/stft_discr.hip and
// csrc/mel_loss.hip.  A workgroup of 4 waves owns a 64 (M) x 64 (N) tile, each wave a 32 x 32 block; the reduction runs in chunks of 32 through LDS
// (A [64][32], B [32][64]), the next chunk's global loads in flight while the matrix core works on the current one.  What differs between the products
// is WHERE an operand element lives, so each product is a small functor: a(m, k), b(k, n), store(m, n, v), all bounds-checked by the kernel (indices
// past M / N / K never reach the functor).  Everything here has internal linkage: each translation unit instantiates the kernel for its own functors.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace {

constexpr int GK = 32;                   // reduction chunk

// a functor with store2(m, n, v0, v1, z) takes rows m (even) and m + 1 of one column in one call: in the accumulator layout of the 32x32 MFMA
// (row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5), column = lane & 31) they are registers v and v + 1 of the same lane, so a product whose rows come in
// pairs -- (re, im) of one frequency -- forms |.|^2 in the epilogue with no exchange.  Such a functor's M is even.
template <class OP, class = void>
struct has_store2 : std::false_type {};
template <class OP>
struct has_store2<OP, std::void_t<decltype(&OP::store2)>> : std::true_type {};

// OP: int M, N; k range [k_lo(z), k_hi(z)); float a(m, k), b(k, n); void store(m, n, v, z); void rowsum(m, v, z) when ROWSUM
template <class OP, bool A_MFAST, bool ROWSUM>
__global__ __launch_bounds__(256) void gemm64_kernel(OP op) {
    __shared__ float As[64][GK + 1];
    __shared__ float Bs[GK][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, z = blockIdx.z;
    const int klo = op.k_lo(z), khi = op.k_hi(z);
    // A: k fastest (k = tid & 31, m = tid >> 5 + 8 i) or m fastest (m = tid & 63, k = tid >> 6 + 4 i);  B: n = tid & 63, k = tid >> 6 + 4 i
    const int a0 = A_MFAST ? (tid & 63) : (tid & 31), a1 = A_MFAST ? (tid >> 6) : (tid >> 5);
    const int bn = n0 + (tid & 63), bk = tid >> 6;
    typename OP::NState ns;
    const bool nok = bn < op.N;
    if (nok) op.decode_n(bn, ns);
    float areg[8], breg[8];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + (A_MFAST ? a0 : a1 + 8 * i), k = k0 + (A_MFAST ? a1 + 4 * i : a0);
            areg[i] = (m < op.M && k < khi) ? op.a(m, k) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + bk + 4 * i;
            breg[i] = (nok && k < khi) ? op.b(k, ns) : 0.f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (A_MFAST) As[a0][a1 + 4 * i] = areg[i];
            else As[a1 + 8 * i][a0] = areg[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) Bs[bk + 4 * i][tid & 63] = breg[i];
    };
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    float rs = 0.f;
    if (klo < khi) {                                             // uniform over the block
        load(klo);
        stage();
        __syncthreads();
        for (int k0 = klo; k0 < khi; k0 += GK) {
            const bool more = k0 + GK < khi;
            if (more) load(k0 + GK);
#pragma unroll
            for (int kk = 0; kk < GK / 2; ++kk)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[wm * 32 + lr][2 * kk + lh], Bs[2 * kk + lh][wn * 32 + lr], acc, 0, 0, 0);
            if (ROWSUM && blockIdx.x == 0 && tid < 64) {
                for (int kk = 0; kk < GK; ++kk) rs += As[tid][kk];
            }
            __syncthreads();
            if (more) {
                stage();
                __syncthreads();
            }
        }
    }
    if constexpr (ROWSUM) {
        if (blockIdx.x == 0 && tid < 64 && m0 + tid < op.M) op.rowsum(m0 + tid, rs, z);
    }
    const int n = n0 + wn * 32 + lr;
    if (n >= op.N) return;
    typename OP::NState os;
    op.decode_n(n, os);
    if constexpr (has_store2<OP>::value) {
#pragma unroll
        for (int v = 0; v < 16; v += 2) {
            const int m = m0 + wm * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
            if (m < op.M) op.store2(m, os, acc[v], acc[v + 1], z);
        }
    } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int m = m0 + wm * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
            if (m < op.M) op.store(m, os, acc[v], z);
        }
    }
}

template <class OP, bool A_MFAST, bool ROWSUM>
int launch_gemm(const OP& op, int splits, hipStream_t st) {
    const dim3 grid((unsigned)((op.N + 63) / 64), (unsigned)((op.M + 63) / 64), (unsigned)splits);
    hipLaunchKernelGGL((gemm64_kernel<OP, A_MFAST, ROWSUM>), grid, dim3(256), 0, st, op);
    ALM_LAUNCH_CHECK();
    return 0;
}

}  // namespace
