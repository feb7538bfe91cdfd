// The denoising SoundStream's two extra pieces for gfx950, forward and backward, exact fp32, no float atomics (every gradient is one fixed-order
// fma / add chain, bitwise reproducible run to run):
//
//   SqueezeExcite inside a ResidualUnit (reference soundstream.py:145-169, 362-369).  Its input there is u [B][C][T] and the module takes the
//   cumulative mean over dim -2, i.e. over the CHANNEL axis, so per column (b, t):
//       m[c]  = (u[0] + ... + u[c]) / (c + 1)
//       z1[j] = b1[j] + sum_c W1[j][c] m[c]        h[j] = silu(z1[j])                 W1 [inner][C]
//       z2[c] = b2[c] + sum_j W2[c][j] h[j]        gate[c] = sigmoid(z2[c])           W2 [C][inner]
//       out[c] = u[c] * gate[c] (+ residual[c])
//   One lane owns one column: lanes run along t (every load / store of u, g, out is a coalesced 256-byte row segment), the running prefix and the
//   `inner` hidden accumulators sit in registers (template NJ = inner rounded up to 8 / 16 / 32 / 64 / 128), the weights are wave-uniform and read
//   through the scalar cache straight from their nn.Conv1d layouts (no derived weight image, so nothing can go stale).  A first sweep over c builds
//   z1, a second one gate and output (u is read twice; the second read of a 64-column tile comes from L2).
//
//   backward: from g = dL/dout and the saved u the same lane recomputes m, z1, h, gate, then
//       dz2[c] = g[c] u[c] gate[c] (1 - gate[c])          dh[j] = sum_c W2[c][j] dz2[c]        dz1[j] = dh[j] silu'(z1[j])
//       dm[c]  = sum_j W1[j][c] dz1[j]                    du[c] = g[c] gate[c] + sum_{c' >= c} dm[c'] / (c' + 1)      (reverse sweep)
//   and leaves m, h, dz2, dz1 in the caller's workspace; the parameter gradients dW1 = sum dz1 m^T, dW2 = sum dz2 h^T, db1, db2 are then two
//   alm_conv1d_wgrad calls (k = 1: per-chunk partial tiles on the exact-fp32 MFMA, summed in chunk order).
//
//   FiLM (soundstream.py:442-449): y[r][c] = x[r][c] gamma[c] + beta[c] on [rows][C], (gamma | beta) = W cond + b with W [2 C][2], cond = (c0, c1).
//   backward: dx = g gamma; dgamma[c] = sum_r g x, dbeta[c] = sum_r g as per-row-chunk partials in the workspace, summed in chunk order by the
//   second launch, which writes dW [2 C][2] = (dgamma | dbeta) (x) cond and db = (dgamma | dbeta).
#include "common.hpp"

namespace {

constexpr int SE_MAX_INNER = 128;

__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }

// grid (ceil(T / 64), B), one wave per workgroup, lane <-> time step
template <int NJ, bool FULL>
__global__ __launch_bounds__(64) void se_gate_fwd_kernel(const float* __restrict__ u, const float* __restrict__ residual, const float* __restrict__ W1,
                                                         const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
                                                         float* __restrict__ out, int C, int inner, int T) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const long long base = (long long)blockIdx.y * C * T + t;
    const float* up = u + base;
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = (FULL || j < inner) ? b1[j] : 0.f;
    float run = 0.f;
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            run += up[(long long)(c + k) * T];
            m[k] = run / (float)(c + k + 1);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (FULL || j < inner) {
                const float* w = W1 + (long long)j * C + c;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j] = fmaf(w[k], m[k], acc[j]);
            }
    }
    for (; c < C; ++c) {
        run += up[(long long)c * T];
        const float m = run / (float)(c + 1);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (FULL || j < inner) acc[j] = fmaf(W1[(long long)j * C + c], m, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = acc[j] * sigmoid_f(acc[j]);          // h = silu(z1); 0 on the padding
    for (c = 0; c < C; c += 4) {
        float z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = c + k < C ? b2[c + k] : 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (FULL || j < inner) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) z[k] = fmaf(W2[(long long)(c + k) * inner + j], acc[j], z[k]);
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < C) {
                const long long o = (long long)(c + k) * T;
                float y = up[o] * sigmoid_f(z[k]);
                if (residual) y += residual[base + o];
                out[base + o] = y;
            }
    }
}

// same grid; writes du [B][C][T] and the four operands of the parameter gradients: m, dz2 [B][C][T], h, dz1 [B][inner][T]
template <int NJ>
__global__ __launch_bounds__(64) void se_gate_bwd_kernel(const float* __restrict__ g, const float* __restrict__ u, const float* __restrict__ W1,
                                                         const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
                                                         float* __restrict__ du, float* __restrict__ m_out, float* __restrict__ h_out,
                                                         float* __restrict__ dz2_out, float* __restrict__ dz1_out, int C, int inner, int T) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const long long base = (long long)blockIdx.y * C * T + t;
    const long long ibase = (long long)blockIdx.y * inner * T + t;
    const float* up = u + base;
    const float* gp = g + base;
    float* dup = du + base;
    float h[NJ], dh[NJ];                                          // 2 NJ registers: silu'(z1) waits in the lane's own dz1 slots meanwhile
#pragma unroll
    for (int j = 0; j < NJ; ++j) h[j] = (j < inner) ? b1[j] : 0.f;
    float run = 0.f;
    for (int c = 0; c < C; c += 4) {                              // sweep 1: the prefix mean (kept for dW1) and z1
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[k] = 0.f;
            if (c + k < C) {
                run += up[(long long)(c + k) * T];
                m[k] = run / (float)(c + k + 1);
                m_out[base + (long long)(c + k) * T] = m[k];
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < inner) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) h[j] = fmaf(W1[(long long)j * C + c + k], m[k], h[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float z = h[j], s = sigmoid_f(z);
        h[j] = z * s;
        dh[j] = 0.f;
        if (j < inner) {
            h_out[ibase + (long long)j * T] = h[j];
            dz1_out[ibase + (long long)j * T] = s * (1.f + z * (1.f - s));          // silu'(z), read back by this lane after sweep 2
        }
    }
    for (int c = 0; c < C; c += 4) {                              // sweep 2: gate, the direct term of du, dz2 and dh
        float z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = c + k < C ? b2[c + k] : 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < inner) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) z[k] = fmaf(W2[(long long)(c + k) * inner + j], h[j], z[k]);
            }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c + k < C) {
                const long long o = (long long)(c + k) * T;
                const float gate = sigmoid_f(z[k]), gv = gp[o];
                dup[o] = gv * gate;
                z[k] = gv * up[o] * gate * (1.f - gate);          // dz2
                dz2_out[base + o] = z[k];
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < inner) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) dh[j] = fmaf(W2[(long long)(c + k) * inner + j], z[k], dh[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j < inner) {
            dh[j] *= dz1_out[ibase + (long long)j * T];           // dz1 = dh silu'(z1)
            dz1_out[ibase + (long long)j * T] = dh[j];
        }
    }
    float suffix = 0.f;
    for (int c = C - 1; c >= 0; --c) {                            // sweep 3, downwards: dm and its reverse suffix sum
        float dm = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < inner) dm = fmaf(W1[(long long)j * C + c], dh[j], dm);
        suffix += dm / (float)(c + 1);
        dup[(long long)c * T] += suffix;                          // this lane wrote the direct term above
    }
}

// thread <-> element of [rows][C]
__global__ __launch_bounds__(256) void film_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                                                       float* __restrict__ y, long long n, int C, float c0, float c1) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float gamma = W[2 * c] * c0 + W[2 * c + 1] * c1 + b[c];
        const float beta = W[2 * (C + c)] * c0 + W[2 * (C + c) + 1] * c1 + b[C + c];
        y[i] = x[i] * gamma + beta;
    }
}

// grid (ceil(C / 64), chunks): lane <-> column, the chunk's rows in order; partials ws [chunk][2][C]
__global__ __launch_bounds__(64) void film_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ W,
                                                      const float* __restrict__ b, float* __restrict__ dx, float* __restrict__ ws, int rows, int C,
                                                      int chunk, float c0, float c1) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const float gamma = W[2 * c] * c0 + W[2 * c + 1] * c1 + b[c];
    const int r0 = blockIdx.y * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    float sg = 0.f, sb = 0.f;
    for (int r = r0; r < r1; ++r) {
        const long long i = (long long)r * C + c;
        const float gv = g[i];
        dx[i] = gv * gamma;
        sg = fmaf(gv, x[i], sg);
        sb += gv;
    }
    ws[((long long)blockIdx.y * 2) * C + c] = sg;
    ws[((long long)blockIdx.y * 2 + 1) * C + c] = sb;
}

__global__ __launch_bounds__(64) void film_bwd_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW, float* __restrict__ db, int C, int NC,
                                                             float c0, float c1) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int k = 0; k < NC; ++k) {
        sg += ws[((long long)k * 2) * C + c];
        sb += ws[((long long)k * 2 + 1) * C + c];
    }
    dW[2 * c] = sg * c0;
    dW[2 * c + 1] = sg * c1;
    dW[2 * (C + c)] = sb * c0;
    dW[2 * (C + c) + 1] = sb * c1;
    db[c] = sg;
    db[C + c] = sb;
}

template <bool FULL>
int se_fwd_launch(int NJ, dim3 grid, hipStream_t st, const float* u, const float* residual, const float* W1, const float* b1, const float* W2,
                  const float* b2, float* out, int C, int inner, int T) {
#define ALM_SE_FWD(N) hipLaunchKernelGGL((se_gate_fwd_kernel<N, FULL>), grid, dim3(64), 0, st, u, residual, W1, b1, W2, b2, out, C, inner, T)
    switch (NJ) {
        case 8: ALM_SE_FWD(8); break;
        case 16: ALM_SE_FWD(16); break;
        case 32: ALM_SE_FWD(32); break;
        case 64: ALM_SE_FWD(64); break;
        default: ALM_SE_FWD(128); break;
    }
#undef ALM_SE_FWD
    ALM_LAUNCH_CHECK();
    return 0;
}

int se_bwd_launch(int NJ, dim3 grid, hipStream_t st, const float* g, const float* u, const float* W1, const float* b1, const float* W2, const float* b2,
                  float* du, float* m, float* h, float* dz2, float* dz1, int C, int inner, int T) {
#define ALM_SE_BWD(N) hipLaunchKernelGGL((se_gate_bwd_kernel<N>), grid, dim3(64), 0, st, g, u, W1, b1, W2, b2, du, m, h, dz2, dz1, C, inner, T)
    switch (NJ) {
        case 8: ALM_SE_BWD(8); break;
        case 16: ALM_SE_BWD(16); break;
        case 32: ALM_SE_BWD(32); break;
        case 64: ALM_SE_BWD(64); break;
        default: ALM_SE_BWD(128); break;
    }
#undef ALM_SE_BWD
    ALM_LAUNCH_CHECK();
    return 0;
}

inline int se_nj(int inner) { return inner <= 8 ? 8 : inner <= 16 ? 16 : inner <= 32 ? 32 : inner <= 64 ? 64 : 128; }

}  // namespace

// 1 iff the squeeze-excite kernels take the widths: any C >= 1, 1 <= inner <= 128 (the hidden accumulators are registers)
extern "C" int alm_se_gate_supported(int C, int inner) { return C >= 1 && inner >= 1 && inner <= SE_MAX_INNER ? 1 : 0; }

extern "C" int alm_se_gate_fwd(const float* u, const float* residual, const float* W1, const float* b1, const float* W2, const float* b2, float* out,
                               int B, int C, int inner, int T, void* stream) {
    if (B <= 0 || C <= 0 || inner <= 0 || T <= 0 || !u || !W1 || !b1 || !W2 || !b2 || !out) return ALM_ERR_BAD_ARG;
    if (!alm_se_gate_supported(C, inner) || B > 65535) return ALM_ERR_UNSUPPORTED;
    const int NJ = se_nj(inner);
    const dim3 grid((unsigned)((T + 63) / 64), (unsigned)B);
    return NJ == inner ? se_fwd_launch<true>(NJ, grid, (hipStream_t)stream, u, residual, W1, b1, W2, b2, out, C, inner, T)
                       : se_fwd_launch<false>(NJ, grid, (hipStream_t)stream, u, residual, W1, b1, W2, b2, out, C, inner, T);
}

// floats of the caller-owned workspace of alm_se_gate_bwd: m and dz2 [B][C][T], h and dz1 [B][inner][T] (each rounded up to 4 floats), then the
// workspaces of the two k = 1 weight-gradient calls; -1 outside the envelope or past 2^31 floats
extern "C" int alm_se_gate_bwd_ws_floats(int B, int C, int inner, int T) {
    if (B <= 0 || C <= 0 || inner <= 0 || T <= 0) return 0;
    if (!alm_se_gate_supported(C, inner) || B > 65535) return -1;
    const int w1 = alm_conv1d_wgrad_ws_floats(B, C, inner, T, 1), w2 = alm_conv1d_wgrad_ws_floats(B, inner, C, T, 1);
    if (w1 < 0 || w2 < 0) return -1;
    const long long n = 2 * up4((long long)B * C * T) + 2 * up4((long long)B * inner * T) + up4(w1) + up4(w2);
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_se_gate_bwd(const float* g, const float* u, const float* W1, const float* b1, const float* W2, const float* b2, float* du, float* dW1,
                               float* db1, float* dW2, float* db2, float* ws, long long ws_floats, int B, int C, int inner, int T, void* stream) {
    if (B <= 0 || C <= 0 || inner <= 0 || T <= 0 || !g || !u || !W1 || !b1 || !W2 || !b2 || !du || !dW1 || !db1 || !dW2 || !db2 || !ws)
        return ALM_ERR_BAD_ARG;
    const int need = alm_se_gate_bwd_ws_floats(B, C, inner, T);
    if (need < 0) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    const long long nc = up4((long long)B * C * T), ni = up4((long long)B * inner * T);
    const int w1 = alm_conv1d_wgrad_ws_floats(B, C, inner, T, 1), w2 = alm_conv1d_wgrad_ws_floats(B, inner, C, T, 1);
    float* m = ws;
    float* dz2 = m + nc;
    float* h = dz2 + nc;
    float* dz1 = h + ni;
    float* ws1 = dz1 + ni;
    float* ws2 = ws1 + up4(w1);
    const int NJ = se_nj(inner);
    const dim3 grid((unsigned)((T + 63) / 64), (unsigned)B);
    const int rc = se_bwd_launch(NJ, grid, (hipStream_t)stream, g, u, W1, b1, W2, b2, du, m, h, dz2, dz1, C, inner, T);
    if (rc) return rc;
    // dW1 [inner][C] = sum dz1 m^T, db1 = sum dz1;  dW2 [C][inner] = sum dz2 h^T, db2 = sum dz2: k = 1 convs' weight gradients
    const int r1 = alm_conv1d_wgrad(dz1, nullptr, m, dW1, db1, ws1, w1, B, C, inner, T, 1, 1, 1, 0, stream);
    if (r1) return r1;
    return alm_conv1d_wgrad(dz2, nullptr, h, dW2, db2, ws2, w2, B, inner, C, T, 1, 1, 1, 0, stream);
}

extern "C" int alm_film_fwd(const float* x, const float* W, const float* b, float* y, int rows, int C, float cond0, float cond1, void* stream) {
    if (rows <= 0 || C <= 0 || !x || !W || !b || !y) return ALM_ERR_BAD_ARG;
    if (C > (1 << 28)) return ALM_ERR_UNSUPPORTED;
    const long long n = (long long)rows * C;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(film_fwd_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, x, W, b, y, n, C, cond0, cond1);
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of alm_film_bwd: row chunks x 2 x C (chunks of 32 rows, doubled until there are at most 1024 of them)
extern "C" int alm_film_bwd_ws_floats(int rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    const int ch = row_chunk(rows, 32, 1024);
    const long long n = (long long)((rows + ch - 1) / ch) * 2 * C;
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_film_bwd(const float* g, const float* x, const float* W, const float* b, float* dx, float* dW, float* db, float* ws,
                            long long ws_floats, int rows, int C, float cond0, float cond1, void* stream) {
    if (rows <= 0 || C <= 0 || !g || !x || !W || !b || !dx || !dW || !db || !ws) return ALM_ERR_BAD_ARG;
    const int need = alm_film_bwd_ws_floats(rows, C);
    if (need < 0 || C > (1 << 28)) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    const int ch = row_chunk(rows, 32, 1024), NC = (rows + ch - 1) / ch;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(film_bwd_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)NC), dim3(64), 0, st, g, x, W, b, dx, ws, rows, C, ch, cond0, cond1);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(film_bwd_reduce_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, ws, dW, db, C, NC, cond0, cond1);
    ALM_LAUNCH_CHECK();
    return 0;
}
