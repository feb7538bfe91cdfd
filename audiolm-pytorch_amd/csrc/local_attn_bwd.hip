// Backward of SoundStream's LocalTransformer pieces that are not GEMMs (forward: local_attn.hip), gfx950, exact fp32, no atomics: every sum has a
// fixed order, so every gradient is bitwise reproducible.  Codec layout [B][C][T] (time = lane axis).
//   * windowed causal attention: two launches.
//       dQ pass     one thread per query like the forward, K / V of the (look-back | own) window pair in LDS as [feature][slot]; sweep 1 recomputes
//                   (m, l), sweep 2 forms dS = p (dO_pre . V - delta) and accumulates the gradient of the rotated query, which the thread carries back
//                   through xpos, rotary, the attention scale, q_scale and the l2-norm.  lse = m + log l and delta go to a [B][H][T] workspace.
//                   With g = sigmoid(gate): dO_pre = g dO, delta = sum_d dO[d] o[d] (o = the saved GATED output), dgate = (1 - g) delta.
//       dK/dV pass  one workgroup per (key window, head, batch), one thread per key.  Key j is seen by the queries j .. min(j + W, T - 1) of the
//                   (own | next) window pair, whose rotated queries and dO_pre sit in LDS as [feature][slot] with lse / delta beside them.  Scores
//                   depend on the slot difference alone, so the queries are rotated as slots of THIS pair and the key once, as slot tid.
//       q_scale / k_scale gradients sum over every (b, h, t): one partial per workgroup (summed over its threads in thread order through LDS), then
//                   a finish launch adds the partials in workgroup order.
//   * LayerNorm backward: dx one thread per (b, t) (mean / rstd recomputed with the forward's arithmetic and left in a [2][B][T] workspace), then
//     dgamma / dbeta one workgroup per channel (thread-strided partial sums + a fixed LDS tree).
//   * GEGLU backward with the forward's erf GELU and its exact derivative.
#include "common.hpp"
#include "launch.hpp"

namespace {

constexpr int LDS_LIMIT = 160 * 1024;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// d/dx [0.5 x (1 + erf(x / sqrt 2))] = cdf + x pdf
__device__ __forceinline__ float gelu_exact_grad_f(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// sums red[d][0 .. W) in thread order for every feature d and writes part[d]; red = [DH][W] floats of LDS, filled by all W threads before the call
template <int DH>
__device__ __forceinline__ void block_feature_sums(const float* red, float* __restrict__ part, int W, int tid) {
    __syncthreads();
    for (int d = tid; d < DH; d += W) {
        float s = 0.f;
        for (int t = 0; t < W; ++t) s += red[d * W + t];
        part[d] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- dQ pass
// grid (windows, H, B), block W.  Writes dqkv's q block, dgates, lse / delta [B][H][T] and the q_scale partial [DH] of this workgroup.
template <int DH>
__global__ __launch_bounds__(256) void local_attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ q_scale, const float* __restrict__ k_scale,
                                                                const float* __restrict__ cos_t, const float* __restrict__ sin_t, const float* __restrict__ xpos_t,
                                                                const float* __restrict__ gates, const float* __restrict__ o, const float* __restrict__ dO,
                                                                float* __restrict__ dqkv, float* __restrict__ dgates, float* __restrict__ lse_ws,
                                                                float* __restrict__ delta_ws, float* __restrict__ qpart, int H, int T, int W, float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S2 = 2 * W;
    float* Kl = lds;                       // [DH][2W]
    float* Vl = lds + DH * S2;             // [DH][2W]
    const int w = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const long long HD = (long long)H * DH;
    const float* qb = qkv + ((long long)b * 3 * HD + (long long)h * DH) * T;
    const float* kb = qb + HD * T;
    const float* vb = kb + HD * T;
    constexpr int HALF = DH / 2;

    // ---- keys / values of the window pair, exactly as the forward builds them: slot s <-> position j = (w - 1) W + s
    for (int s = tid; s < S2; s += W) {
        const long long j = (long long)(w - 1) * W + s;
        if (j < 0 || j >= T) {
#pragma unroll
            for (int d = 0; d < DH; ++d) { Kl[d * S2 + s] = 0.f; Vl[d * S2 + s] = 0.f; }
            continue;
        }
        float kn[DH];
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) { kn[d] = kb[(long long)d * T + j]; ss += kn[d] * kn[d]; }
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int d = 0; d < DH; ++d) kn[d] = kn[d] * inv * k_scale[d];
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            const float rot = d < HALF ? -kn[d + HALF] : kn[d - HALF];
            const float isc = 1.0f / xpos_t[s * DH + d];
            Kl[d * S2 + s] = kn[d] * cos_t[s * DH + d] * isc + rot * sin_t[s * DH + d] * isc;
            Vl[d * S2 + s] = vb[(long long)d * T + j];
        }
    }
    __syncthreads();

    const long long i = (long long)w * W + tid;
    const bool active = i < T;
    const int sq = W + tid;                                                                  // the query's own slot
    float dq[DH];                                                                            // gradient of the rotated query, then of the raw one
#pragma unroll
    for (int d = 0; d < DH; ++d) dq[d] = 0.f;
    if (active) {
        float q[DH], dop[DH];
        {
            float ss = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) { q[d] = qb[(long long)d * T + i]; ss += q[d] * q[d]; }
            const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
            float qn[DH];
#pragma unroll
            for (int d = 0; d < DH; ++d) qn[d] = q[d] * inv * q_scale[d] * scale;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                const float rot = d < HALF ? -qn[d + HALF] : qn[d - HALF];
                const float sc = xpos_t[sq * DH + d];
                q[d] = qn[d] * cos_t[sq * DH + d] * sc + rot * sin_t[sq * DH + d] * sc;
            }
        }
        const long long bht = ((long long)b * H + h) * T + i;
        const float g = sigmoid_f(gates[bht]);
        float delta = 0.f;
        {
            const float* ob = o + ((long long)b * HD + (long long)h * DH) * T + i;
            const float* gb = dO + ((long long)b * HD + (long long)h * DH) * T + i;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                const float go = gb[(long long)d * T];
                delta += go * ob[(long long)d * T];
                dop[d] = g * go;
            }
        }
        // visible keys: 0 <= i - j <= W  <=>  slots max(sq - W, sq - i) .. sq
        int s0 = sq - W;
        if ((long long)(sq - s0) > i) s0 = sq - (int)i;
        float m = -INFINITY, l = 0.f;
        for (int s = s0; s <= sq; ++s) {
            float sim = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) sim += q[d] * Kl[d * S2 + s];
            const float mn = fmaxf(m, sim);
            l = l * expf(m - mn) + expf(sim - mn);
            m = mn;
        }
        const float rl = 1.0f / l;
        for (int s = s0; s <= sq; ++s) {
            float sim = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) { sim += q[d] * Kl[d * S2 + s]; dp += dop[d] * Vl[d * S2 + s]; }
            const float ds = expf(sim - m) * rl * (dp - delta);
#pragma unroll
            for (int d = 0; d < DH; ++d) dq[d] += ds * Kl[d * S2 + s];
        }
        lse_ws[bht] = m + logf(l);
        delta_ws[bht] = delta;
        dgates[bht] = (1.0f - g) * delta;
        // ---- back through xpos and the rotation: qr[d] = qn[d] a[d] + rot(qn)[d] b[d], a = cos xpos, b = sin xpos
#pragma unroll
        for (int d = 0; d < HALF; ++d) {
            const float sc0 = xpos_t[sq * DH + d], sc1 = xpos_t[sq * DH + d + HALF];
            const float a0 = cos_t[sq * DH + d] * sc0, b0 = sin_t[sq * DH + d] * sc0;
            const float a1 = cos_t[sq * DH + d + HALF] * sc1, b1 = sin_t[sq * DH + d + HALF] * sc1;
            const float g0 = dq[d], g1 = dq[d + HALF];
            dq[d] = g0 * a0 + g1 * b1;                                                        // qn[d] enters rot(qn)[d + HALF] with +1
            dq[d + HALF] = g1 * a1 - g0 * b0;                                                 // qn[d + HALF] enters rot(qn)[d] with -1
        }
    }
    __syncthreads();                                                                         // every thread is done with Kl / Vl
    float* red = lds;                                                                        // [DH][W]
    if (active) {
        // ---- back through the attention scale, q_scale and the l2-norm (u = q / |q|, re-read: the rotated q's registers are free again)
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) { const float x = qb[(long long)d * T + i]; ss += x * x; }
        const float nrm = sqrtf(ss);
        const float inv = 1.0f / fmaxf(nrm, 1e-12f);
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            const float u = qb[(long long)d * T + i] * inv;
            red[d * W + tid] = dq[d] * u * scale;                                            // d q_scale[d] of this query
            dq[d] = dq[d] * q_scale[d] * scale;                                              // du[d]
            dot += dq[d] * u;
        }
        if (!(nrm > 1e-12f)) dot = 0.f;                                                      // clamped norm: u = q / eps is linear in q
        float* dqb = dqkv + ((long long)b * 3 * HD + (long long)h * DH) * T + i;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            const float u = qb[(long long)d * T + i] * inv;
            dqb[(long long)d * T] = (dq[d] - u * dot) * inv;
        }
    } else {
#pragma unroll
        for (int d = 0; d < DH; ++d) red[d * W + tid] = 0.f;
    }
    block_feature_sums<DH>(red, qpart + (((long long)b * H + h) * gridDim.x + w) * DH, W, tid);
}

// ---------------------------------------------------------------------------------------------------------------- dK/dV pass
// grid (windows, H, B), block W.  Writes dqkv's k and v blocks and the k_scale partial [DH] of this workgroup.  LDS_STATS: lse / delta of the pair
// sit in LDS; false only where they no longer fit beside Q and dO_pre (dh 64, window 158 .. 160), and then they are read from the workspace.
template <int DH, bool LDS_STATS>
__global__ __launch_bounds__(256) void local_attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ q_scale, const float* __restrict__ k_scale,
                                                                 const float* __restrict__ cos_t, const float* __restrict__ sin_t, const float* __restrict__ xpos_t,
                                                                 const float* __restrict__ gates, const float* __restrict__ dO, const float* __restrict__ lse_ws,
                                                                 const float* __restrict__ delta_ws, float* __restrict__ dqkv, float* __restrict__ kpart,
                                                                 int H, int T, int W, float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S2 = 2 * W;
    float* Ql = lds;                       // [DH][2W] rotated queries of the (own | next) window pair
    float* Dl = lds + DH * S2;             // [DH][2W] dO_pre = sigmoid(gate) dO
    float* Ll = lds + 2 * DH * S2;         // [2W] lse
    float* El = Ll + S2;                   // [2W] delta
    const int w = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const long long HD = (long long)H * DH;
    const float* qb = qkv + ((long long)b * 3 * HD + (long long)h * DH) * T;
    const float* kb = qb + HD * T;
    const float* vb = kb + HD * T;
    const float* gb = dO + ((long long)b * HD + (long long)h * DH) * T;
    const float* Lg = lse_ws + ((long long)b * H + h) * T + (long long)w * W;               // slot s <-> Lg[s], s <= last
    const float* Eg = delta_ws + ((long long)b * H + h) * T + (long long)w * W;
    constexpr int HALF = DH / 2;

    // ---- queries of the window pair: slot s <-> position i = w W + s, rotated as slot s of THIS pair against the key in slot tid.  The forward
    // rotates a query as slot W + (i mod W) of its own (look-back | own) pair and the key as slot W + tid or tid of that pair; the product depends
    // on the slot DIFFERENCE alone (rotary: R(a)^T R(b) = R(b - a); xpos: scale^(s - W) / scale^(tid - W)), which is s - tid either way, so one
    // rotated key serves the queries of both windows (equal up to the rounding of the tables, ~1e-7 relative).
    for (int s = tid; s < S2; s += W) {
        const long long i = (long long)w * W + s;
        if (i >= T) {
#pragma unroll
            for (int d = 0; d < DH; ++d) { Ql[d * S2 + s] = 0.f; Dl[d * S2 + s] = 0.f; }
            if (LDS_STATS) { Ll[s] = 0.f; El[s] = 0.f; }                                     // never read: the query loop stops at the last position
            continue;
        }
        const int sq = s;
        float qn[DH];
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) { qn[d] = qb[(long long)d * T + i]; ss += qn[d] * qn[d]; }
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int d = 0; d < DH; ++d) qn[d] = qn[d] * inv * q_scale[d] * scale;
        const long long bht = ((long long)b * H + h) * T + i;
        const float g = sigmoid_f(gates[bht]);
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            const float rot = d < HALF ? -qn[d + HALF] : qn[d - HALF];
            const float sc = xpos_t[sq * DH + d];
            Ql[d * S2 + s] = qn[d] * cos_t[sq * DH + d] * sc + rot * sin_t[sq * DH + d] * sc;
            Dl[d * S2 + s] = g * gb[(long long)d * T + i];
        }
        if (LDS_STATS) { Ll[s] = lse_ws[bht]; El[s] = delta_ws[bht]; }
    }
    __syncthreads();

    const long long j = (long long)w * W + tid;
    const bool active = j < T;
    const long long rest = (long long)T - 1 - (long long)w * W;                              // slot of the last query of the sequence
    const int last = rest < (long long)(S2 - 1) ? (int)rest : S2 - 1;
    float dk[DH], dv[DH];                                                                    // dk: gradient of the rotated key, then of the raw one
#pragma unroll
    for (int d = 0; d < DH; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
    if (active) {
        float v[DH], kr[DH];
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) { v[d] = vb[(long long)d * T + j]; kr[d] = kb[(long long)d * T + j]; ss += kr[d] * kr[d]; }
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int d = 0; d < DH; ++d) kr[d] = kr[d] * inv * k_scale[d];
#pragma unroll
        for (int d = 0; d < HALF; ++d) {
            const float i0 = 1.0f / xpos_t[tid * DH + d], i1 = 1.0f / xpos_t[tid * DH + d + HALF];
            const float k0 = kr[d], k1 = kr[d + HALF];
            kr[d] = k0 * cos_t[tid * DH + d] * i0 + (-k1) * sin_t[tid * DH + d] * i0;
            kr[d + HALF] = k1 * cos_t[tid * DH + d + HALF] * i1 + k0 * sin_t[tid * DH + d + HALF] * i1;
        }
        const int hi = tid + W < last ? tid + W : last;                                      // queries j .. min(j + W, T - 1) <-> slots tid .. hi
        for (int s = tid; s <= hi; ++s) {
            float sim = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) { sim += Ql[d * S2 + s] * kr[d]; dp += Dl[d * S2 + s] * v[d]; }
            const float p = expf(sim - (LDS_STATS ? Ll[s] : Lg[s]));
            const float ds = p * (dp - (LDS_STATS ? El[s] : Eg[s]));
#pragma unroll
            for (int d = 0; d < DH; ++d) { dv[d] += p * Dl[d * S2 + s]; dk[d] += ds * Ql[d * S2 + s]; }
        }
        // back through xpos (keys: 1 / scale) and the rotation of slot tid
#pragma unroll
        for (int d = 0; d < HALF; ++d) {
            const float i0 = 1.0f / xpos_t[tid * DH + d], i1 = 1.0f / xpos_t[tid * DH + d + HALF];
            const float a0 = cos_t[tid * DH + d] * i0, b0 = sin_t[tid * DH + d] * i0;
            const float a1 = cos_t[tid * DH + d + HALF] * i1, b1 = sin_t[tid * DH + d + HALF] * i1;
            const float g0 = dk[d], g1 = dk[d + HALF];
            dk[d] = g0 * a0 + g1 * b1;
            dk[d + HALF] = g1 * a1 - g0 * b0;
        }
    }
    __syncthreads();                                                                         // every thread is done with Ql / Dl
    float* red = lds;                                                                        // [DH][W]
    if (active) {
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) { const float x = kb[(long long)d * T + j]; ss += x * x; }
        const float nrm = sqrtf(ss);
        const float inv = 1.0f / fmaxf(nrm, 1e-12f);
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            const float u = kb[(long long)d * T + j] * inv;
            red[d * W + tid] = dk[d] * u;                                                    // d k_scale[d] of this key
            dk[d] = dk[d] * k_scale[d];
            dot += dk[d] * u;
        }
        if (!(nrm > 1e-12f)) dot = 0.f;
        float* dkb = dqkv + ((long long)b * 3 * HD + HD + (long long)h * DH) * T + j;
        float* dvb = dkb + HD * T;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            const float u = kb[(long long)d * T + j] * inv;
            dkb[(long long)d * T] = (dk[d] - u * dot) * inv;
            dvb[(long long)d * T] = dv[d];
        }
    } else {
#pragma unroll
        for (int d = 0; d < DH; ++d) red[d * W + tid] = 0.f;
    }
    block_feature_sums<DH>(red, kpart + (((long long)b * H + h) * gridDim.x + w) * DH, W, tid);
}

// dq_scale[d] / dk_scale[d] = the workgroup partials added in workgroup order; block 2 DH: thread d < DH -> q, else k
__global__ __launch_bounds__(128) void local_attn_bwd_finish_kernel(const float* __restrict__ qpart, const float* __restrict__ kpart, float* __restrict__ dq_scale,
                                                                    float* __restrict__ dk_scale, long long P, int DH) {
    const int tid = threadIdx.x;
    const float* part = tid < DH ? qpart : kpart;
    const int d = tid < DH ? tid : tid - DH;
    float s = 0.f;
    for (long long p = 0; p < P; ++p) s += part[p * DH + d];
    (tid < DH ? dq_scale : dk_scale)[d] = s;
}

template <int DH>
int launch_bwd(const float* qkv, const float* q_scale, const float* k_scale, const float* cos_t, const float* sin_t, const float* xpos_t, const float* gates,
               const float* o, const float* dO, float* dqkv, float* dgates, float* dq_scale, float* dk_scale, float* ws, int B, int H, int T, int W,
               float scale, hipStream_t st) {
    const int smem_q = 2 * DH * 2 * W * (int)sizeof(float);
    if (smem_q > LDS_LIMIT) return ALM_ERR_UNSUPPORTED;
    const bool lds_stats = smem_q + 4 * W * (int)sizeof(float) <= LDS_LIMIT;
    const int smem_k = lds_stats ? smem_q + 4 * W * (int)sizeof(float) : smem_q;
    auto kq = local_attn_bwd_dq_kernel<DH>;
    auto kk = lds_stats ? local_attn_bwd_dkv_kernel<DH, true> : local_attn_bwd_dkv_kernel<DH, false>;
    for (const void* f : {reinterpret_cast<const void*>(kq), reinterpret_cast<const void*>(kk)}) {
        const int rc = alm_lds_limit(f, LDS_LIMIT);
        if (rc) return rc;
    }
    const int NW = (T + W - 1) / W;
    const long long BHT = (long long)B * H * T, P = (long long)B * H * NW;
    float* lse = ws;
    float* delta = ws + BHT;
    float* qpart = ws + 2 * BHT;
    float* kpart = qpart + P * DH;
    const dim3 grid(NW, H, B);
    hipLaunchKernelGGL(kq, grid, dim3(W), smem_q, st, qkv, q_scale, k_scale, cos_t, sin_t, xpos_t, gates, o, dO, dqkv, dgates, lse, delta, qpart, H, T, W, scale);
    hipLaunchKernelGGL(kk, grid, dim3(W), smem_k, st, qkv, q_scale, k_scale, cos_t, sin_t, xpos_t, gates, dO, lse, delta, dqkv, kpart, H, T, W, scale);
    hipLaunchKernelGGL(local_attn_bwd_finish_kernel, dim3(1), dim3(2 * DH), 0, st, qpart, kpart, dq_scale, dk_scale, P, DH);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
// dx[b][c][t] = rstd (dxh[c] - mean_c(dxh) - xh[c] mean_c(dxh xh)) (+ residual),  dxh = dy gamma, xh = (x - mean) rstd; one thread per (b, t)
__global__ __launch_bounds__(256) void ln_bct_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ residual, float* __restrict__ dx, float* __restrict__ stats, int C, int T,
                                                            long long BT, float eps) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const long long base = (long long)blockIdx.y * C * T + t;
    const float* xp = x + base;
    const float* gp = dy + base;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int c = 0;
    for (; c + 3 < C; c += 4) {
        s0 += xp[(long long)c * T]; s1 += xp[(long long)(c + 1) * T]; s2 += xp[(long long)(c + 2) * T]; s3 += xp[(long long)(c + 3) * T];
    }
    for (; c < C; ++c) s0 += xp[(long long)c * T];
    const float mean = ((s0 + s1) + (s2 + s3)) / (float)C;
    s0 = s1 = s2 = s3 = 0.f;
    for (c = 0; c + 3 < C; c += 4) {
        const float d0 = xp[(long long)c * T] - mean, d1 = xp[(long long)(c + 1) * T] - mean, d2 = xp[(long long)(c + 2) * T] - mean,
                    d3 = xp[(long long)(c + 3) * T] - mean;
        s0 += d0 * d0; s1 += d1 * d1; s2 += d2 * d2; s3 += d3 * d3;
    }
    for (; c < C; ++c) { const float d = xp[(long long)c * T] - mean; s0 += d * d; }
    const float rstd = 1.0f / sqrtf(((s0 + s1) + (s2 + s3)) / (float)C + eps);
    const long long bt = (long long)blockIdx.y * T + t;
    stats[bt] = mean;
    stats[BT + bt] = rstd;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    for (c = 0; c + 1 < C; c += 2) {
        const float g0 = gp[(long long)c * T] * gamma[c], g1 = gp[(long long)(c + 1) * T] * gamma[c + 1];
        a0 += g0; a1 += g1;
        b0 += g0 * ((xp[(long long)c * T] - mean) * rstd); b1 += g1 * ((xp[(long long)(c + 1) * T] - mean) * rstd);
    }
    for (; c < C; ++c) { const float g0 = gp[(long long)c * T] * gamma[c]; a0 += g0; b0 += g0 * ((xp[(long long)c * T] - mean) * rstd); }
    const float m1 = (a0 + a1) / (float)C, m2 = (b0 + b1) / (float)C;
    float* op = dx + base;
    if (residual) {
        const float* rp = residual + base;
        for (c = 0; c < C; ++c)
            op[(long long)c * T] = rstd * (gp[(long long)c * T] * gamma[c] - m1 - (xp[(long long)c * T] - mean) * rstd * m2) + rp[(long long)c * T];
    } else {
        for (c = 0; c < C; ++c) op[(long long)c * T] = rstd * (gp[(long long)c * T] * gamma[c] - m1 - (xp[(long long)c * T] - mean) * rstd * m2);
    }
}

// dgamma[c] = sum_{b, t} dy xh, dbeta[c] = sum_{b, t} dy: one workgroup per channel, thread-strided sums, then a fixed tree
__global__ __launch_bounds__(256) void ln_bct_bwd_param_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ stats,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta, int C, int T, long long BT) {
    __shared__ float rg[256], rb[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    float sg = 0.f, sb = 0.f;
    for (long long e = tid; e < BT; e += 256) {
        const long long b = e / T, t = e - b * T;
        const long long off = (b * C + c) * T + t;
        const float g = dy[off];
        sg += g * ((x[off] - stats[e]) * stats[BT + e]);
        sb += g;
    }
    rg[tid] = sg; rb[tid] = sb;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) { rg[tid] += rg[tid + n]; rb[tid] += rb[tid + n]; }
        __syncthreads();
    }
    if (tid == 0) { dgamma[c] = rg[0]; dbeta[c] = rb[0]; }
}

// du[b][i][t] = dh gelu(gate), du[b][I + i][t] = dh a gelu'(gate)       (u = [a | gate], h = a gelu(gate))
__global__ __launch_bounds__(256) void geglu_bct_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ u, float* __restrict__ du, int I, long long T,
                                                            long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long bi = e / T, t = e - bi * T;
        const long long b = bi / I, i = bi - b * I;
        const long long ia = (b * 2 * I + i) * T + t, ig = ia + (long long)I * T;
        const float g = dh[e], a = u[ia], gate = u[ig];
        du[ia] = g * gelu_f(gate);
        du[ig] = g * a * gelu_exact_grad_f(gate);
    }
}

}  // namespace

extern "C" int alm_local_attn_bwd_supported(int dim_head, int window) {
    if (dim_head != 32 && dim_head != 64) return 0;
    if (window <= 0 || window > 256) return 0;
    return 2 * dim_head * 2 * window * (int)sizeof(float) <= LDS_LIMIT ? 1 : 0;             // the forward's envelope: K / V of a window pair in LDS
}

extern "C" int alm_local_attn_bwd_ws_floats(int B, int H, int dim_head, int T, int window) {
    if (B <= 0 || H <= 0 || dim_head <= 0 || T <= 0 || window <= 0) return -1;
    const long long NW = ((long long)T + window - 1) / window;
    const long long n = 2LL * B * H * T + 2LL * B * H * NW * dim_head;
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_local_attn_bwd(const float* qkv, const float* q_scale, const float* k_scale, const float* cos_t, const float* sin_t, const float* xpos_t,
                                  const float* gates, const float* o, const float* dO, float* dqkv, float* dgates, float* dq_scale, float* dk_scale, float* ws,
                                  long long ws_floats, int B, int H, int dim_head, int T, int window, float scale, void* stream) {
    if (B <= 0 || H <= 0 || T <= 0 || window <= 0 || !gates || !dgates || !ws) return ALM_ERR_BAD_ARG;
    if (!alm_local_attn_bwd_supported(dim_head, window)) return ALM_ERR_UNSUPPORTED;
    const int need = alm_local_attn_bwd_ws_floats(B, H, dim_head, T, window);
    if (need < 0) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    int rc;
    if (dim_head == 64) rc = launch_bwd<64>(qkv, q_scale, k_scale, cos_t, sin_t, xpos_t, gates, o, dO, dqkv, dgates, dq_scale, dk_scale, ws, B, H, T, window, scale, (hipStream_t)stream);
    else rc = launch_bwd<32>(qkv, q_scale, k_scale, cos_t, sin_t, xpos_t, gates, o, dO, dqkv, dgates, dq_scale, dk_scale, ws, B, H, T, window, scale, (hipStream_t)stream);
    if (rc) return rc;
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_layernorm_bct_bwd_ws_floats(int B, int T) {
    if (B <= 0 || T <= 0) return -1;
    const long long n = 2LL * B * T;
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_layernorm_bct_bwd(const float* dy, const float* x, const float* gamma, const float* residual, float* dx, float* dgamma, float* dbeta,
                                     float* ws, int B, int C, int T, float eps, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0 || !ws || (dgamma == nullptr) != (dbeta == nullptr)) return ALM_ERR_BAD_ARG;
    if (alm_layernorm_bct_bwd_ws_floats(B, T) < 0) return ALM_ERR_UNSUPPORTED;
    const long long BT = (long long)B * T;
    hipLaunchKernelGGL(ln_bct_bwd_dx_kernel, dim3((T + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, residual, dx, ws, C, T, BT, eps);
    if (dgamma) hipLaunchKernelGGL(ln_bct_bwd_param_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, dy, x, ws, dgamma, dbeta, C, T, BT);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_geglu_bct_bwd(const float* dh, const float* u, float* du, int B, int I, int T, void* stream) {
    if (B <= 0 || I <= 0 || T <= 0) return ALM_ERR_BAD_ARG;
    const long long total = (long long)B * I * T;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(geglu_bct_bwd_kernel, dim3((int)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream, dh, u, du, I, (long long)T, total);
    ALM_LAUNCH_CHECK();
    return 0;
}
