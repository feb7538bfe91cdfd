// ComplexSTFTDiscriminator of SoundStream training (reference soundstream.py:173-310), fp32.  Complex tensors are interleaved (re, im) pairs, the
// storage of torch.complex64; every gradient is the pair (dL/dre, dL/dim).  No atomics: every sum has one fixed order.
//
// One implicit-GEMM kernel on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32) carries every matrix product of the module: gemm64_kernel of
// gemm64.hpp (shared with mel_loss.hip), a 64 (M) x 64 (N) tile per workgroup of 4 waves, the loop of conv_valid_kernel in dense_f32.hip.  What differs
// between the products is WHERE an operand element lives, so each product is a small functor: a(m, k), b(k, n), store(m, n, v) (indices past
// M / N / K never reach it).
//   STFT forward   : M = 2 F (f, re | im), N = B T, K = n_fft.  A = the windowed DFT basis [n_fft][2 F] built by the host in float64; B = the frame
//                    sample, reflect padding done by mirroring the index (no padded copy).
//   STFT backward  : frames' gradient [n_fft][B T] = basis x dX (M = n_fft, K = 2 F) into a workspace, then every output sample gathers its own sum
//                    over the <= 3 padded positions that map to it (itself, its mirror at either end) and the frames that cover each, in that order.
//   cconv forward  : [yr; yi] = [Wr -Wi; Wi Wr] [xr; xi]: M = 2 Cout (co, c), N = B Ho Wo, K = 2 Cin kh kw (ci, i, j, d).  The weight is read in the
//                    parameter's layout [Cout][Cin][kh][kw][2]: A(co c, r d) = w[co][r][c ^ d], negated for (c, d) = (0, 1).  + bias (+ residual).
//   cconv dgrad    : M = 2 Cin (ci, d), N = B H W, K = 2 Cout kh kw (co, i, j, c): the transposed block form, a gather over the taps.
//   cconv wgrad    : P(co c, r d) = sum over (b, ho, wo) of g_c x_d: M = 2 Cout, N = 2 Cin kh kw, K = B Ho Wo split over blockIdx.z; each split writes
//                    its P (and, from the tiles of the first column, the row sums = the bias gradient) to its slab of the workspace;
//                    cconv_wgrad_reduce_kernel adds the slabs in split order: dWr = P(0,0) + P(1,1), dWi = P(1,0) - P(0,1).
// ModReLU y = relu(|z| + b) z / |z| and |z|: elementwise, b read from device memory; db of ModReLU in two fixed-order stages.
// Second order (the double backward of the gradient penalty): the backward passes of ModReLU and |z| as functions of (g, z, b), differentiated once
// more against the cotangents (v, beta) of (dz, db) -- elementwise again, the scalar d/db reduced like db.
#include "gemm64.hpp"

namespace {

constexpr int RED_SPAN = 4096, RED_MAX_BLOCKS = 1024;

// ------------------------------------------------------------------------------------------------ STFT

struct StftFwdOp {
    const float* x; const float* basis; float* X;
    int M, N, K, len, hop, pad, F, T;
    struct NState { int b, t, base; };
    __device__ int k_lo(int) const { return 0; }
    __device__ int k_hi(int) const { return K; }
    __device__ void decode_n(int n, NState& s) const { s.b = n / T; s.t = n - s.b * T; s.base = s.t * hop - pad; }
    __device__ float a(int m, int k) const { return basis[(size_t)k * M + m]; }
    __device__ float b(int k, const NState& s) const {
        int pos = s.base + k;
        if (pos < 0) pos = -pos;
        if (pos >= len) pos = 2 * (len - 1) - pos;                // len > n_fft / 2: one reflection lands inside
        return x[(size_t)s.b * len + pos];
    }
    __device__ void store(int m, const NState& s, float v, int) const { X[(((size_t)s.b * F + (m >> 1)) * T + s.t) * 2 + (m & 1)] = v; }
};

struct StftBwdOp {                                                // ws [n_fft][B T] = basis [n_fft][2 F] x dX [2 F][B T]
    const float* dX; const float* basis; float* ws;
    int M, N, K, F, T;
    struct NState { int n; size_t base; };
    __device__ int k_lo(int) const { return 0; }
    __device__ int k_hi(int) const { return K; }
    __device__ void decode_n(int n, NState& s) const { const int b = n / T, t = n - b * T; s.n = n; s.base = ((size_t)b * F * T + t) * 2; }
    __device__ float a(int m, int k) const { return basis[(size_t)m * K + k]; }
    __device__ float b(int k, const NState& s) const { return dX[s.base + (size_t)(k >> 1) * T * 2 + (k & 1)]; }
    __device__ void store(int m, const NState& s, float v, int) const { ws[(size_t)m * N + s.n] = v; }
};

// frames covering padded position q: t hop <= q < t hop + n_fft
__device__ __forceinline__ float ola_at(const float* __restrict__ ws, long long q, int b, int T, int n_fft, int hop, long long NT) {
    long long tlo = q - n_fft + 1;
    tlo = tlo <= 0 ? 0 : (tlo + hop - 1) / hop;
    long long thi = q / hop;
    if (thi > T - 1) thi = T - 1;
    float s = 0.f;
    for (long long t = tlo; t <= thi; ++t) s += ws[(q - t * hop) * NT + (long long)b * T + t];
    return s;
}

__global__ __launch_bounds__(256) void stft_ola_kernel(const float* __restrict__ ws, float* __restrict__ dx, int B, int len, int n_fft, int hop, int T) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * len) return;
    const int b = (int)(i / len), u = (int)(i - (long long)b * len), pad = n_fft / 2;
    const long long NT = (long long)B * T;
    float s = ola_at(ws, (long long)u + pad, b, T, n_fft, hop, NT);
    if (u >= 1 && u <= pad) s += ola_at(ws, (long long)pad - u, b, T, n_fft, hop, NT);                                     // left mirror
    if (u <= len - 2 && u >= len - 1 - pad) s += ola_at(ws, (long long)pad + 2LL * (len - 1) - u, b, T, n_fft, hop, NT);   // right mirror
    dx[i] = s;
}

// ------------------------------------------------------------------------------------------------ complex conv2d

struct CConvGeom { int B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo; };

struct CConvFwdOp {
    const float* x; const float* w; const float* bias; const float* res; float* y;
    CConvGeom g;
    int M, N, K, R, taps;
    struct NState { int b, h0, w0; size_t out; };
    __device__ int k_lo(int) const { return 0; }
    __device__ int k_hi(int) const { return K; }
    __device__ void decode_n(int n, NState& s) const {
        const int hw = g.Ho * g.Wo;
        s.b = n / hw;
        const int r = n - s.b * hw, ho = r / g.Wo, wo = r - ho * g.Wo;
        s.h0 = ho * g.sh - g.ph, s.w0 = wo * g.sw - g.pw;
        s.out = (size_t)s.b * g.Cout * hw + r;
    }
    __device__ float a(int m, int k) const {
        const int c = m & 1, d = k & 1;
        const float v = w[((size_t)(m >> 1) * R + (k >> 1)) * 2 + (c ^ d)];
        return (c == 0 && d == 1) ? -v : v;
    }
    __device__ float b(int k, const NState& s) const {
        const int r = k >> 1, ci = r / taps, tap = r - ci * taps, i = tap / g.kw, j = tap - i * g.kw;
        const int hi = s.h0 + i, wi = s.w0 + j;
        if (hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return 0.f;
        return x[((((size_t)s.b * g.Cin + ci) * g.H + hi) * g.W + wi) * 2 + (k & 1)];
    }
    __device__ void store(int m, const NState& s, float v, int) const {
        const size_t o = (s.out + (size_t)(m >> 1) * g.Ho * g.Wo) * 2 + (m & 1);
        if (bias) v += bias[m];
        if (res) v += res[o];
        y[o] = v;
    }
};

struct CConvDgradOp {
    const float* gy; const float* w; float* dx;
    CConvGeom g;
    int M, N, K, taps;
    struct NState { int b, hp, wp; size_t out; };
    __device__ int k_lo(int) const { return 0; }
    __device__ int k_hi(int) const { return K; }
    __device__ void decode_n(int n, NState& s) const {
        const int hw = g.H * g.W;
        s.b = n / hw;
        const int r = n - s.b * hw, hh = r / g.W, ww = r - hh * g.W;
        s.hp = hh + g.ph, s.wp = ww + g.pw;
        s.out = (size_t)s.b * g.Cin * hw + r;
    }
    __device__ float a(int m, int k) const {
        const int d = m & 1, c = k & 1, r = k >> 1, co = r / taps, tap = r - co * taps;
        const float v = w[(((size_t)co * g.Cin + (m >> 1)) * taps + tap) * 2 + (c ^ d)];
        return (c == 0 && d == 1) ? -v : v;
    }
    __device__ float b(int k, const NState& s) const {
        const int r = k >> 1, co = r / taps, tap = r - co * taps, i = tap / g.kw, j = tap - i * g.kw;
        const int th = s.hp - i, tw = s.wp - j;
        if (th < 0 || tw < 0) return 0.f;
        const int ho = th / g.sh, wo = tw / g.sw;
        if (ho * g.sh != th || wo * g.sw != tw || ho >= g.Ho || wo >= g.Wo) return 0.f;
        return gy[((((size_t)s.b * g.Cout + co) * g.Ho + ho) * g.Wo + wo) * 2 + (k & 1)];
    }
    __device__ void store(int m, const NState& s, float v, int) const { dx[(s.out + (size_t)(m >> 1) * g.H * g.W) * 2 + (m & 1)] = v; }
};

struct CConvWgradOp {
    const float* gy; const float* x; float* ws;
    CConvGeom g;
    int M, N, K, taps, per;                                       // per: reduction elements per split (a multiple of GK)
    struct NState { int n, ci, i, j, d; };
    __device__ int k_lo(int z) const { return z * per; }
    __device__ int k_hi(int z) const { return min(K, (z + 1) * per); }
    __device__ void decode_n(int n, NState& s) const {
        const int r = n >> 1;
        s.n = n, s.d = n & 1, s.ci = r / taps;
        const int tap = r - s.ci * taps;
        s.i = tap / g.kw, s.j = tap - s.i * g.kw;
    }
    __device__ float a(int m, int k) const {
        const int hw = g.Ho * g.Wo, b = k / hw, r = k - b * hw;
        return gy[(((size_t)b * g.Cout + (m >> 1)) * hw + r) * 2 + (m & 1)];
    }
    __device__ float b(int k, const NState& s) const {
        const int hw = g.Ho * g.Wo, b = k / hw, r = k - b * hw, ho = r / g.Wo, wo = r - ho * g.Wo;
        const int hi = ho * g.sh - g.ph + s.i, wi = wo * g.sw - g.pw + s.j;
        if (hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return 0.f;
        return x[((((size_t)b * g.Cin + s.ci) * g.H + hi) * g.W + wi) * 2 + s.d];
    }
    __device__ float* slab(int z) const { return ws + (size_t)z * ((size_t)M * N + M); }
    __device__ void store(int m, const NState& s, float v, int z) const { slab(z)[(size_t)m * N + s.n] = v; }
    __device__ void rowsum(int m, float v, int z) const { slab(z)[(size_t)M * N + m] = v; }
};

// dw [Cout][R][2], db [Cout][2] from the splits' slabs [M = 2 Cout][N = 2 R] (+ M row sums), in split order
__global__ __launch_bounds__(256) void cconv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, int Cout, int R,
                                                                 int splits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long M = 2LL * Cout, N = 2LL * R, ndw = M * R, slab = M * N + M;
    if (i >= ndw + M) return;
    float s = 0.f;
    if (i < ndw) {
        const long long e = i & 1, cr = i >> 1, co = cr / R, r = cr - co * R;
        const long long p0 = e ? (2 * co + 1) * N + 2 * r : (2 * co) * N + 2 * r;               // dWr: P(0,0) + P(1,1);  dWi: P(1,0) - P(0,1)
        const long long p1 = e ? (2 * co) * N + 2 * r + 1 : (2 * co + 1) * N + 2 * r + 1;
        for (int sp = 0; sp < splits; ++sp) {
            const float* p = ws + (size_t)sp * slab;
            s += e ? p[p0] - p[p1] : p[p0] + p[p1];
        }
        dw[i] = s;
    } else {
        for (int sp = 0; sp < splits; ++sp) s += ws[(size_t)sp * slab + M * N + (i - ndw)];
        db[i - ndw] = s;
    }
}

bool geom_ok(const CConvGeom& g) {
    return g.B > 0 && g.Cin > 0 && g.Cout > 0 && g.H > 0 && g.W > 0 && g.kh > 0 && g.kw > 0 && g.sh > 0 && g.sw > 0 && g.ph >= 0 && g.pw >= 0 &&
           (long long)g.H + 2LL * g.ph >= g.kh && (long long)g.W + 2LL * g.pw >= g.kw;
}

constexpr long long I31 = 0x7fffffffLL;

// every flattened GEMM index is 32-bit; tensor offsets are size_t
bool geom_fits(const CConvGeom& g) {
    const long long taps = (long long)g.kh * g.kw;
    if (taps >= I31 || (long long)g.H + g.ph + g.kh >= I31 || (long long)g.W + g.pw + g.kw >= I31) return false;
    if ((long long)g.H * g.sh >= I31 || (long long)g.W * g.sw >= I31) return false;
    const long long nin = (long long)g.B * g.H * g.W, nout = (long long)g.B * g.Ho * g.Wo;
    if ((long long)g.H * g.W >= I31 || nin + 64 >= I31 || nout + 64 >= I31) return false;
    if (2LL * g.Cin * taps + 64 >= I31 || 2LL * g.Cout * taps + 64 >= I31) return false;
    return (2LL * g.Cin + 63) / 64 <= 65535 && (2LL * g.Cout + 63) / 64 <= 65535;
}

CConvGeom make_geom(int B, int Cin, int Cout, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw) {
    CConvGeom g = {B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw, 0, 0};
    if (geom_ok(g)) {
        g.Ho = (int)(((long long)H + 2LL * ph - kh) / sh + 1);
        g.Wo = (int)(((long long)W + 2LL * pw - kw) / sw + 1);
    }
    return g;
}

struct CWgPlan { int per, splits; long long slab; };

bool cwgrad_plan(const CConvGeom& g, CWgPlan& p) {
    if (!geom_ok(g) || !geom_fits(g)) return false;
    const long long M = 2LL * g.Cout, N = 2LL * g.Cin * g.kh * g.kw, K = (long long)g.B * g.Ho * g.Wo;
    const long long tiles = ((M + 63) / 64) * ((N + 63) / 64);
    if ((N + 63) / 64 >= I31) return false;
    long long want = (1024 + tiles - 1) / tiles;                   // ~1024 blocks in flight; a function of the shapes only
    if (want > 256) want = 256;
    const long long chunks = (K + GK - 1) / GK;
    if (want > chunks) want = chunks;
    const long long per = (chunks + want - 1) / want;
    p.per = (int)(per * GK);
    p.splits = (int)((chunks + per - 1) / per);
    p.slab = M * N + M;
    return (long long)p.splits * p.slab < I31 && K + p.per < I31;
}

// ------------------------------------------------------------------------------------------------ ModReLU, |z|

__global__ __launch_bounds__(256) void modrelu_fwd_kernel(const float2* __restrict__ z, const float* __restrict__ bp, float2* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float b = bp[0];
    const float2 v = z[i];
    const float r = hypotf(v.x, v.y), a = fmaxf(r + b, 0.f);
    float2 o;
    if (r > 0.f) o.x = a * (v.x / r), o.y = a * (v.y / r);
    else o.x = a, o.y = 0.f;                                       // angle(0) = 0
    y[i] = o;
}

// dz elementwise; this block's share of db (a contiguous span, fixed lane order) into part[blockIdx.x]
__global__ __launch_bounds__(256) void modrelu_bwd_kernel(const float2* __restrict__ g, const float2* __restrict__ z, const float* __restrict__ bp,
                                                          float2* __restrict__ dz, float* __restrict__ part, long long n, long long span) {
    const long long lo = (long long)blockIdx.x * span, hi = min(n, lo + span);
    const float b = bp[0];
    float s = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const float2 v = z[i], gv = g[i];
        const float r = hypotf(v.x, v.y);
        float2 o = {0.f, 0.f};
        if (r + b > 0.f) {
            if (r > 0.f) {
                const float ux = v.x / r, uy = v.y / r, ug = ux * gv.x + uy * gv.y, q = b / r;
                o.x = gv.x + q * (gv.x - ux * ug);
                o.y = gv.y + q * (gv.y - uy * ug);
                s += ug;
            } else {
                s += gv.x;
            }
        }
        if (dz) dz[i] = o;
    }
    s = block_sum(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The backward above as a function: dz = g + (b / r) P g, db = sum u . g where r + b > 0 (u = z / r, P = I - u u^T on (re, im) pairs).  With
// S = <v, dz> + beta db:  dS/dg = v + (b / r) P v + beta u,  dS/db = sum <v, P g> / r,
// dS/dz = -(b / r^2) (<v, P g> u + (u . g) P v + (u . v) P g) + (beta / r) P g.  At r = 0 the backward is dz = 0, db += g_re: dS/dg = (beta, 0).
// v may be null (dz was not asked for: its cotangent is zero).
__global__ __launch_bounds__(256) void modrelu_bwd2_kernel(const float2* __restrict__ g, const float2* __restrict__ z, const float* __restrict__ bp,
                                                           const float2* __restrict__ v, const float* __restrict__ betap, float2* __restrict__ dg,
                                                           float2* __restrict__ dz, float* __restrict__ part, long long n, long long span) {
    const long long lo = (long long)blockIdx.x * span, hi = min(n, lo + span);
    const float b = bp[0], beta = betap[0];
    float s = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const float2 zv = z[i], gv = g[i];
        const float2 vv = v ? v[i] : make_float2(0.f, 0.f);
        const float r = hypotf(zv.x, zv.y);
        float2 og = {0.f, 0.f}, oz = {0.f, 0.f};
        if (r + b > 0.f) {
            if (r > 0.f) {
                const float ux = zv.x / r, uy = zv.y / r, ug = ux * gv.x + uy * gv.y, uv = ux * vv.x + uy * vv.y, q = b / r;
                const float pgx = gv.x - ux * ug, pgy = gv.y - uy * ug, pvx = vv.x - ux * uv, pvy = vv.y - uy * uv;
                const float vpg = vv.x * pgx + vv.y * pgy, br = beta / r, q2 = q / r;
                og.x = vv.x + q * pvx + beta * ux;
                og.y = vv.y + q * pvy + beta * uy;
                oz.x = br * pgx - q2 * (vpg * ux + ug * pvx + uv * pgx);
                oz.y = br * pgy - q2 * (vpg * uy + ug * pvy + uv * pgy);
                s += vpg / r;
            } else {
                og.x = beta;
            }
        }
        dg[i] = og;
        if (dz) dz[i] = oz;
    }
    s = block_sum(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(256) void cabs_fwd_kernel(const float2* __restrict__ z, float* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = hypotf(z[i].x, z[i].y);
}

__global__ __launch_bounds__(256) void cabs_bwd_kernel(const float* __restrict__ g, const float2* __restrict__ z, float2* __restrict__ dz, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 v = z[i];
    const float r = hypotf(v.x, v.y);
    float2 o = {0.f, 0.f};
    if (r > 0.f) o.x = g[i] * (v.x / r), o.y = g[i] * (v.y / r);
    dz[i] = o;
}

// dz = g u as a function of (g, z), against the cotangent v of dz: dS/dg = u . v, dS/dz = g P v / r; both 0 at r = 0
__global__ __launch_bounds__(256) void cabs_bwd2_kernel(const float* __restrict__ g, const float2* __restrict__ z, const float2* __restrict__ v,
                                                        float* __restrict__ dg, float2* __restrict__ dz, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 zv = z[i], vv = v[i];
    const float r = hypotf(zv.x, zv.y);
    float og = 0.f;
    float2 oz = {0.f, 0.f};
    if (r > 0.f) {
        const float ux = zv.x / r, uy = zv.y / r, uv = ux * vv.x + uy * vv.y, q = g[i] / r;
        og = uv;
        oz.x = q * (vv.x - ux * uv), oz.y = q * (vv.y - uy * uv);
    }
    dg[i] = og;
    if (dz) dz[i] = oz;
}

bool stft_ok(int B, int n, int n_fft, int hop, int F) { return B > 0 && n > 0 && n_fft > 0 && hop > 0 && F > 0 && F <= n_fft; }

}  // namespace

extern "C" int alm_stft_frames(int n, int n_fft, int hop) {
    if (n <= 0 || n_fft <= 0 || hop <= 0 || n <= n_fft / 2) return -1;
    return (int)(((long long)n + 2LL * (n_fft / 2) - n_fft) / hop + 1);
}

extern "C" int alm_stft_fwd(const float* x, const float* basis, float* X, int B, int n, int n_fft, int hop, int F, void* stream) {
    if (!stft_ok(B, n, n_fft, hop, F)) return ALM_ERR_BAD_ARG;
    const int T = alm_stft_frames(n, n_fft, hop);
    if (T < 1 || (long long)B * T + 64 >= I31 || (long long)n + 2LL * n_fft >= I31 || (long long)T * hop >= I31 || (2LL * F + 63) / 64 > 65535)
        return ALM_ERR_UNSUPPORTED;
    StftFwdOp op = {x, basis, X, 2 * F, B * T, n_fft, n, hop, n_fft / 2, F, T};
    return launch_gemm<StftFwdOp, true, false>(op, 1, (hipStream_t)stream);
}

// floats of the caller-owned workspace of alm_stft_bwd: the frames' gradient [n_fft][B T]; -1 outside the kernel's envelope
extern "C" int alm_stft_bwd_ws_floats(int B, int n, int n_fft, int hop) {
    const int T = alm_stft_frames(n, n_fft, hop);
    if (B <= 0 || T < 1) return -1;
    const long long f = (long long)n_fft * B * T;
    return f >= I31 ? -1 : (int)f;
}

extern "C" int alm_stft_bwd(const float* dX, const float* basis, float* dx, float* ws, long long ws_floats, int B, int n, int n_fft, int hop, int F,
                            void* stream) {
    if (!stft_ok(B, n, n_fft, hop, F)) return ALM_ERR_BAD_ARG;
    const int T = alm_stft_frames(n, n_fft, hop);
    if (T < 1 || (long long)B * T + 64 >= I31 || (long long)n + 2LL * n_fft >= I31 || (long long)T * hop >= I31 || (n_fft + 63) / 64 > 65535 ||
        ((long long)B * n + 255) / 256 >= I31)
        return ALM_ERR_UNSUPPORTED;
    if (ws_floats < (long long)n_fft * B * T) return ALM_ERR_BAD_ARG;
    StftBwdOp op = {dX, basis, ws, n_fft, B * T, 2 * F, F, T};
    const int rc = launch_gemm<StftBwdOp, false, false>(op, 1, (hipStream_t)stream);
    if (rc) return rc;
    hipLaunchKernelGGL(stft_ola_kernel, dim3((unsigned)(((long long)B * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, dx, B, n, n_fft, hop, T);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_cconv2d_out_hw(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int* Ho, int* Wo) {
    const CConvGeom g = make_geom(1, 1, 1, H, W, kh, kw, sh, sw, ph, pw);
    if (!geom_ok(g)) return -1;
    if (Ho) *Ho = g.Ho;
    if (Wo) *Wo = g.Wo;
    return 0;
}

extern "C" int alm_cconv2d_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int Cin, int Cout, int H, int W,
                               int kh, int kw, int sh, int sw, int ph, int pw, void* stream) {
    const CConvGeom g = make_geom(B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw);
    if (!geom_ok(g)) return ALM_ERR_BAD_ARG;
    if (!geom_fits(g)) return ALM_ERR_UNSUPPORTED;
    CConvFwdOp op = {x, w, bias, residual, y, g, 2 * Cout, B * g.Ho * g.Wo, 2 * Cin * kh * kw, Cin * kh * kw, kh * kw};
    return launch_gemm<CConvFwdOp, false, false>(op, 1, (hipStream_t)stream);
}

extern "C" int alm_cconv2d_dgrad(const float* g_, const float* w, float* dx, int B, int Cin, int Cout, int H, int W, int kh, int kw, int sh, int sw, int ph,
                                 int pw, void* stream) {
    const CConvGeom g = make_geom(B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw);
    if (!geom_ok(g)) return ALM_ERR_BAD_ARG;
    if (!geom_fits(g)) return ALM_ERR_UNSUPPORTED;
    CConvDgradOp op = {g_, w, dx, g, 2 * Cin, B * H * W, 2 * Cout * kh * kw, kh * kw};
    return launch_gemm<CConvDgradOp, false, false>(op, 1, (hipStream_t)stream);
}

// floats of the caller-owned workspace of alm_cconv2d_wgrad: splits x (2 Cout x 2 Cin kh kw + 2 Cout); -1 outside the kernel's envelope
extern "C" int alm_cconv2d_wgrad_ws_floats(int B, int Cin, int Cout, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw) {
    CWgPlan p;
    if (!cwgrad_plan(make_geom(B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw), p)) return -1;
    return (int)(p.splits * p.slab);
}

extern "C" int alm_cconv2d_wgrad(const float* g_, const float* x, float* dw, float* db, float* ws, long long ws_floats, int B, int Cin, int Cout, int H,
                                 int W, int kh, int kw, int sh, int sw, int ph, int pw, void* stream) {
    const CConvGeom g = make_geom(B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw);
    if (!geom_ok(g)) return ALM_ERR_BAD_ARG;
    CWgPlan p;
    if (!cwgrad_plan(g, p)) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < p.splits * p.slab) return ALM_ERR_BAD_ARG;
    const int R = Cin * kh * kw;
    CConvWgradOp op = {g_, x, ws, g, 2 * Cout, 2 * R, B * g.Ho * g.Wo, kh * kw, p.per};
    const int rc = launch_gemm<CConvWgradOp, false, true>(op, p.splits, (hipStream_t)stream);
    if (rc) return rc;
    const long long n = 2LL * Cout * R + 2LL * Cout;
    hipLaunchKernelGGL(cconv_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, dw, db, Cout, R, p.splits);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_modrelu_ws_floats(void) { return RED_MAX_BLOCKS; }

extern "C" int alm_modrelu_fwd(const float* z, const float* b, float* y, long long n, void* stream) {
    if (n <= 0) return ALM_ERR_BAD_ARG;
    if ((n + 255) / 256 >= I31) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(modrelu_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float2*)z, b, (float2*)y, n);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_modrelu_bwd(const float* g, const float* z, const float* b, float* dz, float* db, float* ws, long long n, void* stream) {
    if (n <= 0 || db == nullptr || ws == nullptr) return ALM_ERR_BAD_ARG;
    long long span = RED_SPAN;
    while ((n + span - 1) / span > RED_MAX_BLOCKS) span *= 2;
    const int nparts = (int)((n + span - 1) / span);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(modrelu_bwd_kernel, dim3(nparts), dim3(256), 0, st, (const float2*)g, (const float2*)z, b, (float2*)dz, ws, n, span);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, st, ws, db, nparts);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_modrelu_bwd2(const float* g, const float* z, const float* b, const float* v, const float* beta, float* dg, float* dz, float* db,
                                float* ws, long long n, void* stream) {
    if (g == nullptr || z == nullptr || b == nullptr || beta == nullptr || dg == nullptr || db == nullptr || ws == nullptr || n <= 0) return ALM_ERR_BAD_ARG;
    long long span = RED_SPAN;
    while ((n + span - 1) / span > RED_MAX_BLOCKS) span *= 2;
    const int nparts = (int)((n + span - 1) / span);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(modrelu_bwd2_kernel, dim3(nparts), dim3(256), 0, st, (const float2*)g, (const float2*)z, b, (const float2*)v, beta, (float2*)dg,
                       (float2*)dz, ws, n, span);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, st, ws, db, nparts);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_cabs_fwd(const float* z, float* y, long long n, void* stream) {
    if (n <= 0) return ALM_ERR_BAD_ARG;
    if ((n + 255) / 256 >= I31) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cabs_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float2*)z, y, n);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_cabs_bwd(const float* g, const float* z, float* dz, long long n, void* stream) {
    if (n <= 0) return ALM_ERR_BAD_ARG;
    if ((n + 255) / 256 >= I31) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cabs_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, (const float2*)z, (float2*)dz, n);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_cabs_bwd2(const float* g, const float* z, const float* v, float* dg, float* dz, long long n, void* stream) {
    if (g == nullptr || z == nullptr || v == nullptr || dg == nullptr || n <= 0) return ALM_ERR_BAD_ARG;
    if ((n + 255) / 256 >= I31) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cabs_bwd2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, (const float2*)z, (const float2*)v, dg,
                       (float2*)dz, n);
    ALM_LAUNCH_CHECK();
    return 0;
}
