// Backward of SoundStream's causal conv stacks for gfx950 (reference soundstream.py:332-395, 519-531, 615-627), exact fp32 on
// v_mfma_f32_32x32x2_f32 like the forward (csrc/conv1d.hpp).  No float atomics anywhere: every gradient is one fixed-order fma / add chain, bitwise
// reproducible run to run.
//
// Conventions of the forward: x [B][Cin][Tin], out / g = dL/dout [B][Cout][Tout], W [Cout][Cin][k], pad = dil (k - 1) + 1 - stride,
// out[co][t] = sum_{tap, ci} W[co][ci][tap] * xpad[ci][t * stride + tap * dil], xpad[p] = x[p - pad] for p >= pad and x[pad - p] (reflect) or 0
// (zero_pad) left of it.
//
//   ELU backward, fused into every load of g:  g_pre = g * (y > 0 ? 1 : y + 1), y = the saved post-ELU output (ELU' = exp(v) = y + 1 for v <= 0).
//
//   dgrad : dx[ci][i] = dxp[pad + i] + (1 <= i <= pad, reflect ? dxp[pad - i] : 0),
//           dxp[ci][pp] = sum_{tap, co} W[co][ci][tap] * g_pre[co][t]  over the (t, tap) with t * stride + tap * dil = pp.
//           Both terms meet the SAME tap weight, so the B operand of one MFMA is g_pre[t1] + g_pre[t2] (t1 the direct, t2 the mirrored step, each 0
//           where it does not exist) and the fold costs no second pass and no atomic.  Time is the MFMA column / lane axis as in the forward.  A
//           workgroup owns ONE output phase r = i mod stride (lane q <-> i = q * stride + r): whether tap contributes is then wave-uniform
//           ((pad + r - tap * dil) mod stride == 0), so a stride-s down-sampling conv (k = 2 s) runs 2 of its 2 s taps per phase instead of masking
//           lanes -- the phase form of CausalConvTranspose1d.forward.  The A operand is the transposed weight image [tap][co][ci]
//           (alm_conv1d_pack of W^T, once per weight version).  An optional residual is added in the epilogue (the skip path of a ResidualUnit).
//   wgrad : dW[co][ci][tap] = sum_{b, t} g_pre[co][t] * xpad[ci][t * stride + tap * dil], db[co] = sum_{b, t} g_pre[co][t]: a GEMM whose contraction
//           runs over B * Tout (millions at the first stage) against 32 x 32 outputs.  Time is cut into chunks (alm_conv1d_wgrad_chunk steps, never
//           across batch elements); one workgroup per (chunk, 32 co x 32 ci tile, tap group) writes fp32 partial tiles into the caller's workspace
//           (alm_conv1d_wgrad_ws_floats), conv1d_wgrad_reduce_kernel then sums the partials in chunk order.  Both operands are contiguous along
//           time while the MFMA wants the channel on the lane axis: the tiles go through LDS (coalesced row loads in, transposed reads out).
//   Cin = 1 / Cout = 1 (first encoder conv, last decoder conv) run the same kernels on a zero-padded 32-channel tile.
#include "common.hpp"

namespace {

struct DgradArgs {
    const float* g; const float* y; const float* wt; const float* residual; float* dx;
    int B, Cin, CinP, Cout, CoutP, Tin, Tout, ks, stride, dil, pad, zero_pad;
};

__device__ __forceinline__ int pmod(int a, int m) { const int r = a % m; return r < 0 ? r + m : r; }

// grid: (ceil(ceil(Tin / stride) / 256), CinP / 32, B * stride); 4 waves along q, 64 q each (two 32-column MFMA blocks)
__global__ __launch_bounds__(256) void conv1d_dgrad_kernel(DgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int b = blockIdx.z / a.stride, r = blockIdx.z % a.stride;
    const int ci0 = blockIdx.y * 32;
    const int q0 = blockIdx.x * 256 + wave * 64;
    if (q0 * a.stride + r >= a.Tin) return;                          // wave-uniform: nothing of this phase left
    const long long gb = (long long)b * a.Cout * a.Tout;
    const auto rsG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g + gb), 0, a.Cout * a.Tout * 4, 0x00020000);
    const auto rsY = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.y ? a.y + gb : a.g + gb), 0, a.Cout * a.Tout * 4, 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wt), 0, a.ks * a.CoutP * a.CinP * 4, 0x00020000);
    const bool has_y = a.y != nullptr;

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    int i[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) i[j] = (q0 + j * 32 + lr) * a.stride + r;
    const bool fold = !a.zero_pad && a.pad > 0 && q0 * a.stride + r <= a.pad;      // wave-uniform: some lane has 1 <= i <= pad
    const int OOB = (int)0x80000000;
    const int nk = a.CoutP >> 1;                                     // co pairs
    for (int tap = 0; tap < a.ks; ++tap) {
        const bool v1 = pmod(a.pad + r - tap * a.dil, a.stride) == 0;
        const bool v2 = fold && pmod(a.pad - r - tap * a.dil, a.stride) == 0;
        if (!v1 && !v2) continue;
        int o1[2], o2[2];                                            // byte offsets of the direct / mirrored step inside channel lh (OOB: reads 0)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n1 = a.pad + i[j] - tap * a.dil, n2 = a.pad - i[j] - tap * a.dil;
            const int t1 = n1 / a.stride, t2 = n2 / a.stride;
            o1[j] = (v1 && i[j] < a.Tin && n1 >= 0 && t1 < a.Tout) ? (lh * a.Tout + t1) * 4 : OOB;
            o2[j] = (v2 && i[j] >= 1 && i[j] <= a.pad && i[j] < a.Tin && n2 >= 0 && t2 < a.Tout) ? (lh * a.Tout + t2) * 4 : OOB;
        }
        const int wvo = ((tap * a.CoutP + lh) * a.CinP + ci0 + lr) * 4;
        for (int k = 0; k < nk; ++k) {
            const int so = 2 * k * a.Tout * 4;
            const float av = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsW, wvo, 2 * k * a.CinP * 4, 0));
            float bv[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float g1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsG, o1[j], so, 0));
                float g2 = 0.f;
                if (v2) g2 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsG, o2[j], so, 0));
                if (has_y) {
                    const float y1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsY, o1[j], so, 0));
                    g1 *= y1 > 0.f ? 1.f : y1 + 1.f;
                    if (v2) {
                        const float y2 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsY, o2[j], so, 0));
                        g2 *= y2 > 0.f ? 1.f : y2 + 1.f;
                    }
                }
                bv[j] = g1 + g2;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[j], acc[j], 0, 0, 0);
        }
    }
    // D layout: column = lane & 31 (time), row = (e & 3) + 8 * (e >> 2) + 4 * lh (input channel)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (i[j] >= a.Tin) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ci = ci0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (ci < a.Cin) {
                const long long o = ((long long)b * a.Cin + ci) * a.Tin + i[j];
                float v = acc[j][e];
                if (a.residual) v += a.residual[o];
                a.dx[o] = v;
            }
        }
    }
}

struct WgradArgs {
    const float* g; const float* y; const float* x; float* ws;
    int B, Cin, CinP, Cout, CoutP, Tin, Tout, ks, stride, dil, pad, zero_pad, chunk, nch, NC;
};

// grid: (NC chunks, (CoutP / 32) * (CinP / 32) channel tiles, ceil(ks / TG) tap groups).  A workgroup walks its chunk in 64-step slabs.  Per slab the 256
// threads load the g_pre tile [32 co][64 t] and the x tile(s) [32 ci][...] with coalesced row loads (time contiguous, the index map of the forward's
// pad applied on the way) into LDS rows of ODD length, and every wave reads its MFMA operands back "transposed" (lane = channel, conflict-free):
// wave w contracts steps 16 w .. 16 w + 15 of the slab for all TG taps.  HALO (stride 1): ONE x tile of 64 + (taps - 1) dil columns serves every tap
// (tap tt reads it shifted by tt dil); otherwise one [32][64] tile per tap.  At the end the four waves' accumulators are summed through LDS in wave
// order and the tile is written to this chunk's slot of the workspace; threads 0..31 of the (tap group 0, ci tile 0) workgroups sum g_pre per channel.
constexpr int WG_LD = 65, WG_XS = 4 * 32 * WG_LD;

template <int TG, bool HALO>
__global__ __launch_bounds__(256, 2) void conv1d_wgrad_kernel(WgradArgs a) {
    __shared__ float gs[32 * WG_LD];
    __shared__ float xs[WG_XS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int c = blockIdx.x;
    const int nci = a.CinP >> 5;
    const int co0 = (blockIdx.y / nci) * 32, ci0 = (blockIdx.y % nci) * 32;
    const int tap0 = blockIdx.z * TG;
    const int ntap = a.ks - tap0 < TG ? a.ks - tap0 : TG;
    const int b = c / a.nch, tc0 = (c % a.nch) * a.chunk;
    const int tc1 = tc0 + a.chunk < a.Tout ? tc0 + a.chunk : a.Tout;
    const float* gB = a.g + (long long)b * a.Cout * a.Tout;
    const float* yB = a.y ? a.y + (long long)b * a.Cout * a.Tout : nullptr;
    const float* xB = a.x + (long long)b * a.Cin * a.Tin;
    const bool do_db = blockIdx.z == 0 && ci0 == 0;
    const int W = 64 + (ntap - 1) * a.dil, ldw = W | 1;              // HALO tile: columns and (odd) row length
    const int lrow = tid >> 6, lcol = tid & 63;

    f32x16 acc[TG];
#pragma unroll
    for (int tt = 0; tt < TG; ++tt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tt][e] = 0.f;
    float bsum = 0.f;

    auto load_x = [&](int ci, int q) {                               // x at padded-time index q - pad already subtracted: reflect / zero left of 0
        const bool left = q < 0;
        q = left ? -q : q;
        return (ci < a.Cin && q < a.Tin && !(left && a.zero_pad)) ? xB[(long long)ci * a.Tin + q] : 0.f;
    };

    for (int tg = tc0; tg < tc1; tg += 64) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = lrow + 4 * p, co = co0 + row, t = tg + lcol;
            float v = 0.f;
            if (co < a.Cout && t < tc1) {
                v = gB[(long long)co * a.Tout + t];
                if (yB) {
                    const float yv = yB[(long long)co * a.Tout + t];
                    v *= yv > 0.f ? 1.f : yv + 1.f;
                }
            }
            gs[row * WG_LD + lcol] = v;
        }
        if constexpr (HALO) {
            const int q0 = tg - a.pad + tap0 * a.dil;                // stride 1: step t, tap tt reads x[t + (tap0 + tt) dil - pad]
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int row = lrow + 4 * p;
                for (int w = lcol; w < W; w += 64) xs[row * ldw + w] = load_x(ci0 + row, q0 + w);
            }
        } else {
            for (int tt = 0; tt < ntap; ++tt)
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int row = lrow + 4 * p;
                    xs[(tt * 32 + row) * WG_LD + lcol] = load_x(ci0 + row, (tg + lcol) * a.stride + (tap0 + tt) * a.dil - a.pad);
                }
        }
        __syncthreads();
        if (do_db && tid < 32) {
            for (int j = 0; j < 64; ++j) bsum += gs[tid * WG_LD + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int tl = wave * 16 + lh * 8 + j;                   // k = 0 <-> step 16 w + j, k = 1 <-> step 16 w + 8 + j, for A and B alike
            const float av = gs[lr * WG_LD + tl];
#pragma unroll
            for (int tt = 0; tt < TG; ++tt)
                if (tt < ntap) {
                    const float bv = HALO ? xs[lr * ldw + tl + tt * a.dil] : xs[(tt * 32 + lr) * WG_LD + tl];
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tt], 0, 0, 0);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int tt = 0; tt < TG; ++tt)
        if (tt < ntap) {
#pragma unroll
            for (int e = 0; e < 16; ++e) xs[wave * 1024 + ((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + lr] = acc[tt][e];
            __syncthreads();
            float* wsT = a.ws + ((long long)c * a.ks + tap0 + tt) * a.CoutP * a.CinP;
            for (int i = tid; i < 1024; i += 256) {
                const float s = ((xs[i] + xs[1024 + i]) + xs[2048 + i]) + xs[3072 + i];
                wsT[(long long)(co0 + (i >> 5)) * a.CinP + ci0 + (i & 31)] = s;
            }
            __syncthreads();
        }
    if (do_db && tid < 32) a.ws[(long long)a.NC * a.ks * a.CoutP * a.CinP + (long long)c * a.CoutP + co0 + tid] = bsum;
}

// dW[co][ci][tap] = sum over chunks, in chunk order; db[co] likewise (threads past the weight elements)
__global__ __launch_bounds__(256) void conv1d_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, int Cin,
                                                                   int CinP, int Cout, int CoutP, int ks, int NC) {
    const long long nw = (long long)ks * Cout * Cin;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        const int ci = (int)(i % Cin), co = (int)((i / Cin) % Cout), tap = (int)(i / ((long long)Cin * Cout));
        const float* p = ws + ((long long)tap * CoutP + co) * CinP + ci;
        const long long ld = (long long)ks * CoutP * CinP;
        float s = 0.f;
#pragma unroll 8
        for (int c = 0; c < NC; ++c) s += p[c * ld];
        dw[((long long)co * Cin + ci) * ks + tap] = s;
    } else if (i < nw + Cout) {
        const int co = (int)(i - nw);
        const float* p = ws + (long long)NC * ks * CoutP * CinP + co;
        float s = 0.f;
#pragma unroll 8
        for (int c = 0; c < NC; ++c) s += p[(long long)c * CoutP];
        db[co] = s;
    }
}

// adjoint of phase_interleave_kernel: g[b][co][q * s + r] -> y[b][r * Cout + co][q]
__global__ __launch_bounds__(256) void phase_deinterleave_kernel(const float* __restrict__ g, float* __restrict__ y, int Cout, int s, int n) {
    const long long total = (long long)s * Cout * n;
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int q = (int)(i % n);
        const int co = (int)((i / n) % Cout);
        const int r = (int)(i / ((long long)n * Cout));
        y[(long long)b * total + i] = g[((long long)b * Cout + co) * n * s + (long long)q * s + r];
    }
}

}  // namespace

// time steps per weight-gradient chunk: 2048, or 8192 once that would make more than 512 chunks (the first stages of a long batch)
extern "C" int alm_conv1d_wgrad_chunk(int B, int Tout) {
    if (B <= 0 || Tout <= 0) return 0;
    return (long long)B * ((Tout + 2047) / 2048) <= 512 ? 2048 : 8192;
}

// floats of the caller-owned workspace of alm_conv1d_wgrad: chunks x (ksize x CoutP x CinP partial tiles + CoutP bias partials), channels padded to 32;
// -1 when that does not fit an int (ALM_ERR_UNSUPPORTED from the launch)
extern "C" int alm_conv1d_wgrad_ws_floats(int B, int Cin, int Cout, int Tout, int ksize) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Tout <= 0 || ksize <= 0) return 0;
    const int ch = alm_conv1d_wgrad_chunk(B, Tout);
    const long long NC = (long long)B * ((Tout + ch - 1) / ch);
    const long long CinP = (Cin + 31) & ~31, CoutP = (Cout + 31) & ~31;
    const long long n = NC * (ksize * CoutP * CinP + CoutP);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_conv1d_dgrad(const float* g, const float* y, const float* wt, const float* residual, float* dx, int B, int Cin, int Cout, int Tin,
                                int ksize, int stride, int dilation, int zero_pad, void* stream) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Tin <= 0 || ksize <= 0 || stride <= 0 || dilation <= 0) return ALM_ERR_BAD_ARG;
    const int pad = dilation * (ksize - 1) + 1 - stride;
    if (pad < 0 || pad >= Tin || Tin < stride) return ALM_ERR_UNSUPPORTED;
    const int Tout = (Tin - stride) / stride + 1;
    const int CinP = (Cin + 31) & ~31, CoutP = (Cout + 1) & ~1;
    if ((long long)(Cout + 2) * Tout * 4 >= 0x7fffffffLL || (long long)ksize * CoutP * CinP * 4 >= 0x7fffffffLL || (long long)B * stride > 65535 ||
        (long long)Tin + pad + (long long)ksize * dilation >= 0x3fffffffLL)
        return ALM_ERR_UNSUPPORTED;                                                  // 32-bit buffer offsets, grid z
    DgradArgs a{g, y, wt, residual, dx, B, Cin, CinP, Cout, CoutP, Tin, Tout, ksize, stride, dilation, pad, zero_pad};
    const int nq = (Tin + stride - 1) / stride;
    hipLaunchKernelGGL(conv1d_dgrad_kernel, dim3((nq + 255) / 256, CinP / 32, B * stride), dim3(256), 0, (hipStream_t)stream, a);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_conv1d_wgrad(const float* g, const float* y, const float* x, float* dw, float* db, float* ws, long long ws_floats, int B, int Cin,
                                int Cout, int Tin, int ksize, int stride, int dilation, int zero_pad, void* stream) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Tin <= 0 || ksize <= 0 || stride <= 0 || dilation <= 0) return ALM_ERR_BAD_ARG;
    const int pad = dilation * (ksize - 1) + 1 - stride;
    if (pad < 0 || pad >= Tin || Tin < stride) return ALM_ERR_UNSUPPORTED;
    const int Tout = (Tin - stride) / stride + 1;
    const int need = alm_conv1d_wgrad_ws_floats(B, Cin, Cout, Tout, ksize);
    if (need < 0) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    const int CinP = (Cin + 31) & ~31, CoutP = (Cout + 31) & ~31;
    const int ch = alm_conv1d_wgrad_chunk(B, Tout), nch = (Tout + ch - 1) / ch;
    const long long NC = (long long)B * nch;
    const long long tiles = (long long)(CoutP / 32) * (CinP / 32);
    if (NC >= 0x7fffffffLL || tiles > 65535 || ksize > 65535 || (long long)Tin + pad + (long long)ksize * dilation >= 0x3fffffffLL) return ALM_ERR_UNSUPPORTED;
    WgradArgs a{g, y, x, ws, B, Cin, CinP, Cout, CoutP, Tin, Tout, ksize, stride, dilation, pad, zero_pad, ch, nch, (int)NC};
    hipStream_t st = (hipStream_t)stream;
    // stride 1: one x tile with a (taps - 1) dil halo serves up to 8 taps, if its 32 rows fit the LDS buffer; else one tile per tap, 4 taps per workgroup
    const auto halo_fits = [&](int tg) { return 32 * ((64 + ((ksize < tg ? ksize : tg) - 1) * dilation) | 1) <= WG_XS; };
    if (stride == 1 && ksize <= 2 && halo_fits(2)) {
        hipLaunchKernelGGL((conv1d_wgrad_kernel<2, true>), dim3((unsigned)NC, (unsigned)tiles, (ksize + 1) / 2), dim3(256), 0, st, a);
    } else if (stride == 1 && halo_fits(8)) {
        hipLaunchKernelGGL((conv1d_wgrad_kernel<8, true>), dim3((unsigned)NC, (unsigned)tiles, (ksize + 7) / 8), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((conv1d_wgrad_kernel<4, false>), dim3((unsigned)NC, (unsigned)tiles, (ksize + 3) / 4), dim3(256), 0, st, a);
    }
    ALM_LAUNCH_CHECK();
    const long long n = (long long)ksize * Cout * Cin + Cout;
    hipLaunchKernelGGL(conv1d_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, dw, db, Cin, CinP, Cout, CoutP, ksize, (int)NC);
    ALM_LAUNCH_CHECK();
    return 0;
}

// g [B][Cout][n * s] -> y [B][s * Cout][n] (phase-major channels): the adjoint of alm_phase_interleave
extern "C" int alm_phase_deinterleave(const float* g, float* y, int B, int Cout, int s, int n, void* stream) {
    if (B <= 0 || Cout <= 0 || s <= 0 || n <= 0) return ALM_ERR_BAD_ARG;
    if (B > 65535) return ALM_ERR_UNSUPPORTED;
    const long long total = (long long)Cout * n * s;
    const int gx = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(phase_deinterleave_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, g, y, Cout, s, n);
    ALM_LAUNCH_CHECK();
    return 0;
}
