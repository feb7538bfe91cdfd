// Gate-loop layer of SoundStream(use_gate_loop_layers=True) (reference soundstream.py:524-525, 620-621: Residual(ChannelTranspose(GateLoop(c)))), restated
// in tests/gate_loop_restated.py.  Codec layout [B][C][T] fp32, time contiguous; exact fp32, no atomics, every reduction in a fixed order.
//
//   r[b,t] = sqrt(C) / max(||x[b,:,t]||, 1e-12);  xn = x r gamma                 alm_gate_loop_norm_fwd
//   z = W xn  (k = 1 conv on the exact-fp32 MFMA path, alm_conv1d_causal)        z [B][3 C][T]: q | kv | a rows
//   h[t] = sigmoid(z_a[t]) h[t-1] + z_kv[t], h[-1] = 0;  y = z_q h + 2 x          alm_gate_loop_scan_fwd
//
// The scan composes the affine maps h -> a h + kv along time.  A workgroup of 256 lanes owns one CHUNK of GL_CHUNK = 4096 consecutive steps of one
// (b, channel) row, as 4 tiles of 1024: a lane composes 4 consecutive steps (one 16-byte load per operand where the row start allows), a 64-lane shuffle
// scan composes the lanes' maps, the 4 waves' totals meet in LDS and the tile's end state is carried to the next tile.  The chunk length is a constant
// of the source: the association order of a row depends on T only, never on the device or the launch.  Rows of at most one chunk take ONE launch.
// Longer rows take three: chunk aggregates, one lane per row walking the chunks in order (the carries), then the same scan again with its carry-in.
// No workgroup ever waits for another one.
//
// Backward: dh[t] = g[t] q[t] + a[t+1] dh[t+1] is the same scan run from the row's end with the gate shifted by one step (alm_gate_loop_scan_bwd, which
// reads h from a forward scan in `h only` mode); then the k = 1 conv's input / weight gradients (alm_conv1d_dgrad / alm_conv1d_wgrad), then
// alm_gate_loop_norm_bwd: dx = r gamma dxn - x (r^3 / C) sum_k dxn_k gamma_k x_k + 2 g, dgamma from per-block partials added in block order.
#include "common.hpp"

namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_TILE = GL_THREADS * 4;          // steps per tile: 4 consecutive steps per lane
constexpr int GL_TILES = 4;
constexpr int GL_CHUNK = GL_TILE * GL_TILES;     // steps per workgroup
constexpr int GL_NCOLS = 512;                    // columns per workgroup of the norm backward (8 sub-tiles of 64)

struct Aff { float p, s; };                      // the map h -> p h + s

// `later` after `earlier`
__device__ __forceinline__ Aff compose(Aff earlier, Aff later) { return Aff{later.p * earlier.p, fmaf(later.p, earlier.s, later.s)}; }

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

// Every lane hands in the composition `loc` of its own steps; lanes are in scan order (lane 0 of wave 0 first).  Returns the composition of everything
// before the lane's first step since the chunk's start, `carry` included, and advances `carry` (uniform over the workgroup) to the tile's end.
// sh: 4 Aff of this tile's parity (double-buffered by the caller, so that one barrier per tile is enough).
__device__ __forceinline__ Aff tile_prefix(Aff loc, Aff& carry, Aff* sh, int lane, int wave) {
    Aff inc = loc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Aff prev{__shfl_up(inc.p, d, 64), __shfl_up(inc.s, d, 64)};
        if (lane >= d) inc = compose(prev, inc);
    }
    if (lane == 63) sh[wave] = inc;
    Aff ex{__shfl_up(inc.p, 1, 64), __shfl_up(inc.s, 1, 64)};
    if (lane == 0) ex = Aff{1.f, 0.f};
    __syncthreads();
    Aff pre = carry, tot = carry;
#pragma unroll
    for (int w = 0; w < GL_THREADS / 64; ++w) {
        const Aff t = sh[w];
        tot = compose(tot, t);
        if (w < wave) pre = compose(pre, t);
    }
    carry = tot;
    return compose(pre, ex);
}

__device__ __forceinline__ void load4(const float* __restrict__ row, long long t0, int T, bool vec, float fill, float (&v)[4]) {
    if (vec) {
        if (t0 < T) {
            const float4 f = *reinterpret_cast<const float4*>(row + t0);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
            v[0] = v[1] = v[2] = v[3] = fill;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = t0 + j < T ? row[t0 + j] : fill;
    }
}

__device__ __forceinline__ void store4(float* __restrict__ row, long long t0, int T, bool vec, const float (&v)[4]) {
    if (vec) {
        if (t0 < T) *reinterpret_cast<float4*>(row + t0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t0 + j < T) row[t0 + j] = v[j];
    }
}

// MODE 0: out = z_q h + 2 x;  1: out = h;  2: agg[row][chunk] = the chunk's composed map, nothing else written.
// grid: rows * NC workgroups (row-major); carry_in [rows][NC] = h before each chunk, or NULL (rows of one chunk: h = 0)
template <int MODE, bool VEC>
__global__ __launch_bounds__(GL_THREADS) void gl_scan_fwd_kernel(const float* __restrict__ z, const float* __restrict__ x, float* __restrict__ out,
                                                                 const float* __restrict__ carry_in, float* __restrict__ agg, int C, int T, int NC) {
    __shared__ Aff sh[2][GL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x / NC;
    const int chunk = blockIdx.x % NC;
    const long long b = row / C, c = row % C;
    const float* zq = z + (b * 3 * C + c) * T;
    const float* zkv = zq + (long long)C * T;
    const float* za = zkv + (long long)C * T;
    Aff carry = MODE == 2 ? Aff{1.f, 0.f} : Aff{0.f, carry_in ? carry_in[row * NC + chunk] : 0.f};
    for (int i = 0; i < GL_TILES; ++i) {
        const long long base = (long long)chunk * GL_CHUNK + (long long)i * GL_TILE;
        if (base >= T) break;
        const long long t0 = base + tid * 4;
        float a[4], kv[4];
        load4(za, t0, T, VEC, 0.f, a);
        load4(zkv, t0, T, VEC, 0.f, kv);
        Aff loc{1.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = t0 + j < T ? sigmoid_f(a[j]) : 1.f;                 // past the row's end: the identity map
            loc = compose(loc, Aff{a[j], kv[j]});
        }
        const Aff pre = tile_prefix(loc, carry, sh[i & 1], lane, wave);
        if (MODE == 2) continue;
        float h = pre.s, o[4];
        if (MODE == 0) {
            float q[4], xv[4];
            load4(zq, t0, T, VEC, 0.f, q);
            load4(x + row * T, t0, T, VEC, 0.f, xv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h = fmaf(a[j], h, kv[j]);
                o[j] = fmaf(q[j], h, 2.f * xv[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h = fmaf(a[j], h, kv[j]);
                o[j] = h;
            }
        }
        store4(out + row * T, t0, T, VEC, o);
    }
    if (MODE == 2 && tid == 0) {
        agg[2 * (row * NC + chunk)] = carry.p;
        agg[2 * (row * NC + chunk) + 1] = carry.s;
    }
}

// one lane per row: carry[row][chunk] = the state entering each chunk, walking the chunks in scan order (rev: from the row's end)
__global__ __launch_bounds__(64) void gl_carry_kernel(const float* __restrict__ agg, float* __restrict__ carry, long long rows, int NC, int rev) {
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    float h = 0.f;
    for (int k = 0; k < NC; ++k) {
        const long long i = row * NC + (rev ? NC - 1 - k : k);
        carry[i] = h;
        h = fmaf(agg[2 * i], h, agg[2 * i + 1]);
    }
}

// The reverse scan dh[t] = g[t] q[t] + a[t+1] dh[t+1] (a[T] = 0) over the same chunks, tiles and lanes as the forward scan, walked from the end: lane `tid`
// owns step group 255 - tid of its tile.  AGG: agg[row][chunk] only.  Otherwise dz rows: dq = g h, dkv = dh, da = dh h[t-1] a (1 - a), exactly 0 at t = 0.
template <bool AGG, bool VEC>
__global__ __launch_bounds__(GL_THREADS) void gl_scan_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z, const float* __restrict__ h,
                                                                 float* __restrict__ dz, const float* __restrict__ carry_in, float* __restrict__ agg,
                                                                 int C, int T, int NC) {
    __shared__ Aff sh[2][GL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x / NC;
    const int chunk = blockIdx.x % NC;
    const long long b = row / C, c = row % C;
    const long long oq = (b * 3 * C + c) * T, okv = oq + (long long)C * T, oa = okv + (long long)C * T;
    const float* zq = z + oq;
    const float* za = z + oa;
    const float* gr = g + row * T;
    const float* hr = AGG ? nullptr : h + row * T;
    Aff carry = AGG ? Aff{1.f, 0.f} : Aff{0.f, carry_in ? carry_in[row * NC + chunk] : 0.f};
    for (int i = GL_TILES - 1; i >= 0; --i) {
        const long long base = (long long)chunk * GL_CHUNK + (long long)i * GL_TILE;
        if (base >= T) continue;
        const long long t0 = base + (GL_THREADS - 1 - tid) * 4;
        float a[4], q[4], gv[4], gate[4], val[4];
        load4(za, t0, T, VEC, 0.f, a);
        load4(zq, t0, T, VEC, 0.f, q);
        load4(gr, t0, T, VEC, 0.f, gv);
        const float a_next = t0 + 4 < T ? sigmoid_f(za[t0 + 4]) : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = sigmoid_f(a[j]);
        Aff loc{1.f, 0.f};
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const float nxt = j == 3 ? a_next : a[j + 1];
            gate[j] = t0 + j < T ? (t0 + j + 1 < T ? nxt : 0.f) : 1.f;      // past the row's end: the identity map; the last step: a[T] = 0
            val[j] = t0 + j < T ? gv[j] * q[j] : 0.f;
            loc = compose(loc, Aff{gate[j], val[j]});
        }
        const Aff pre = tile_prefix(loc, carry, sh[i & 1], lane, wave);
        if (AGG) continue;
        float hv[4], dq[4], dkv[4], da[4];
        load4(hr, t0, T, VEC, 0.f, hv);
        const float h_prev = t0 > 0 && t0 <= T ? hr[t0 - 1] : 0.f;
        float dh = pre.s;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            dh = fmaf(gate[j], dh, val[j]);
            const float hp = j == 0 ? h_prev : hv[j - 1];
            dq[j] = gv[j] * hv[j];
            dkv[j] = dh;
            da[j] = t0 + j == 0 ? 0.f : dh * hp * (a[j] * (1.f - a[j]));
        }
        store4(dz + oq, t0, T, VEC, dq);
        store4(dz + okv, t0, T, VEC, dkv);
        store4(dz + oa, t0, T, VEC, da);
    }
    if (AGG && tid == 0) {
        agg[2 * (row * NC + chunk)] = carry.p;
        agg[2 * (row * NC + chunk) + 1] = carry.s;
    }
}

// RMSNorm over the channel axis.  grid ((T + 63) / 64, B), 256 lanes: lane = column, wave w = channels w, w + 4, ...; the 4 partial sums of squares
// meet in LDS and are added in wave order
__global__ __launch_bounds__(256) void gl_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, float* __restrict__ xn, int C,
                                                          int T) {
    __shared__ float sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = (long long)blockIdx.x * 64 + lane;
    const bool live = t < T;
    const float* xb = x + (long long)blockIdx.y * C * T + t;
    float* ob = xn + (long long)blockIdx.y * C * T + t;
    float ss = 0.f;
    if (live)
        for (int c = wave; c < C; c += 4) {
            const float v = xb[(long long)c * T];
            ss = fmaf(v, v, ss);
        }
    sh[wave][lane] = ss;
    __syncthreads();
    const float tot = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
    const float r = sqrtf((float)C) / fmaxf(sqrtf(tot), 1e-12f);
    if (live)
        for (int c = wave; c < C; c += 4) ob[(long long)c * T] = xb[(long long)c * T] * r * gamma[c];
}

// grid ((T + 511) / 512, B), 256 lanes.  Pass 1: per column sum x^2 and sum_k dxn_k gamma_k x_k (wave w = channels w, w + 4, ...; the 4 partials added
// in wave order) -> r and the coefficient of x.  Pass 2: dx, and per channel the block's partial of dgamma = sum dxn x r (a lane adds its 8 columns in
// order, then a fixed butterfly over the 64 lanes) -> part[block][C]
__global__ __launch_bounds__(256) void gl_norm_bwd_kernel(const float* __restrict__ dxn, const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ g, float* __restrict__ dx, float* __restrict__ part, int C, int T) {
    __shared__ float s_ss[4][GL_NCOLS], s_dot[4][GL_NCOLS], s_r[GL_NCOLS], s_k[GL_NCOLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tb = (long long)blockIdx.x * GL_NCOLS;
    const long long off = (long long)blockIdx.y * C * T;
    for (int s = 0; s < GL_NCOLS / 64; ++s) {
        const long long t = tb + s * 64 + lane;
        float ss = 0.f, dot = 0.f;
        if (t < T)
            for (int c = wave; c < C; c += 4) {
                const long long i = off + (long long)c * T + t;
                const float v = x[i];
                ss = fmaf(v, v, ss);
                dot = fmaf(dxn[i] * gamma[c], v, dot);
            }
        s_ss[wave][s * 64 + lane] = ss;
        s_dot[wave][s * 64 + lane] = dot;
    }
    __syncthreads();
    for (int col = threadIdx.x; col < GL_NCOLS; col += 256) {
        const float tot = ((s_ss[0][col] + s_ss[1][col]) + s_ss[2][col]) + s_ss[3][col];
        const float dot = ((s_dot[0][col] + s_dot[1][col]) + s_dot[2][col]) + s_dot[3][col];
        const float nrm = sqrtf(tot);
        const float r = sqrtf((float)C) / fmaxf(nrm, 1e-12f);
        s_r[col] = r;
        s_k[col] = nrm < 1e-12f ? 0.f : r * r / (float)C * r * dot;       // below the clamp r is a constant: no second term
    }
    __syncthreads();
    float* pb = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * C;
    for (int c = wave; c < C; c += 4) {
        const float gm = gamma[c];
        float acc = 0.f;
        for (int s = 0; s < GL_NCOLS / 64; ++s) {
            const long long t = tb + s * 64 + lane;
            if (t < T) {
                const long long i = off + (long long)c * T + t;
                const float v = x[i], d = dxn[i], r = s_r[s * 64 + lane];
                dx[i] = fmaf(r * gm, d, fmaf(-v, s_k[s * 64 + lane], 2.f * g[i]));
                acc = fmaf(d * v, r, acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) pb[c] = acc;
    }
}

__global__ __launch_bounds__(64) void gl_dgamma_kernel(const float* __restrict__ part, float* __restrict__ dgamma, int C, int NB) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int k = 0; k < NB; ++k) s += part[(long long)k * C + c];
    dgamma[c] = s;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline long long gl_chunks(int T) { return ((long long)T + GL_CHUNK - 1) / GL_CHUNK; }

}  // namespace

extern "C" int alm_gate_loop_chunk(void) { return GL_CHUNK; }

extern "C" int alm_gate_loop_norm_fwd(const float* x, const float* gamma, float* xn, int B, int C, int T, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0 || !x || !gamma || !xn) return ALM_ERR_BAD_ARG;
    if (B > 65535) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gl_norm_fwd_kernel, dim3((unsigned)(((long long)T + 63) / 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, gamma, xn, C, T);
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of the two scans: nothing for rows of at most one chunk, else per (row, chunk) the composed map (2) and the
// carry (1); -1 past 2^31 - 1 workgroups or floats
extern "C" int alm_gate_loop_scan_ws_floats(int B, int C, int T) {
    if (B <= 0 || C <= 0 || T <= 0) return 0;
    const long long nc = gl_chunks(T), wgs = (long long)B * C * nc;
    if (wgs > 0x7fffffffLL || 3 * wgs > 0x7fffffffLL) return -1;
    return nc == 1 ? 0 : (int)(3 * wgs);
}

extern "C" int alm_gate_loop_scan_fwd(const float* z, const float* x, float* out, float* ws, long long ws_floats, int B, int C, int T, int h_only,
                                      void* stream) {
    if (B <= 0 || C <= 0 || T <= 0 || !z || !out || (!h_only && !x)) return ALM_ERR_BAD_ARG;
    const int need = alm_gate_loop_scan_ws_floats(B, C, T);
    if (need < 0) return ALM_ERR_UNSUPPORTED;
    if (need > 0 && (!ws || ws_floats < need)) return ALM_ERR_BAD_ARG;
    const long long rows = (long long)B * C;
    const int NC = (int)gl_chunks(T);
    const dim3 grid((unsigned)(rows * NC)), blk(GL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = T % 4 == 0 && aligned16(z) && aligned16(out) && (h_only || aligned16(x));
    float* agg = ws;
    float* carry = NC > 1 ? ws + 2 * rows * NC : nullptr;
#define ALM_GL_FWD(MODE, CARRY, AGG)                                                                                                            \
    do {                                                                                                                                         \
        if (vec) hipLaunchKernelGGL((gl_scan_fwd_kernel<MODE, true>), grid, blk, 0, st, z, x, out, (const float*)(CARRY), AGG, C, T, NC);        \
        else hipLaunchKernelGGL((gl_scan_fwd_kernel<MODE, false>), grid, blk, 0, st, z, x, out, (const float*)(CARRY), AGG, C, T, NC);           \
        ALM_LAUNCH_CHECK();                                                                                                                      \
    } while (0)
    if (NC > 1) {
        ALM_GL_FWD(2, nullptr, agg);
        hipLaunchKernelGGL(gl_carry_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, (const float*)agg, carry, rows, NC, 0);
        ALM_LAUNCH_CHECK();
    }
    if (h_only) ALM_GL_FWD(1, carry, (float*)nullptr);
    else ALM_GL_FWD(0, carry, (float*)nullptr);
#undef ALM_GL_FWD
    return 0;
}

extern "C" int alm_gate_loop_scan_bwd(const float* g, const float* z, const float* h, float* dz, float* ws, long long ws_floats, int B, int C, int T,
                                      void* stream) {
    if (B <= 0 || C <= 0 || T <= 0 || !g || !z || !h || !dz) return ALM_ERR_BAD_ARG;
    const int need = alm_gate_loop_scan_ws_floats(B, C, T);
    if (need < 0) return ALM_ERR_UNSUPPORTED;
    if (need > 0 && (!ws || ws_floats < need)) return ALM_ERR_BAD_ARG;
    const long long rows = (long long)B * C;
    const int NC = (int)gl_chunks(T);
    const dim3 grid((unsigned)(rows * NC)), blk(GL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = T % 4 == 0 && aligned16(g) && aligned16(z) && aligned16(h) && aligned16(dz);
    float* agg = ws;
    float* carry = NC > 1 ? ws + 2 * rows * NC : nullptr;
    if (NC > 1) {
        if (vec) hipLaunchKernelGGL((gl_scan_bwd_kernel<true, true>), grid, blk, 0, st, g, z, h, dz, (const float*)nullptr, agg, C, T, NC);
        else hipLaunchKernelGGL((gl_scan_bwd_kernel<true, false>), grid, blk, 0, st, g, z, h, dz, (const float*)nullptr, agg, C, T, NC);
        ALM_LAUNCH_CHECK();
        hipLaunchKernelGGL(gl_carry_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, (const float*)agg, carry, rows, NC, 1);
        ALM_LAUNCH_CHECK();
    }
    if (vec) hipLaunchKernelGGL((gl_scan_bwd_kernel<false, true>), grid, blk, 0, st, g, z, h, dz, (const float*)carry, (float*)nullptr, C, T, NC);
    else hipLaunchKernelGGL((gl_scan_bwd_kernel<false, false>), grid, blk, 0, st, g, z, h, dz, (const float*)carry, (float*)nullptr, C, T, NC);
    ALM_LAUNCH_CHECK();
    return 0;
}

// floats of the caller-owned workspace of alm_gate_loop_norm_bwd: B x ceil(T / 512) blocks x C partials of dgamma; -1 past 2^31 - 1 floats
extern "C" int alm_gate_loop_norm_bwd_ws_floats(int B, int C, int T) {
    if (B <= 0 || C <= 0 || T <= 0) return 0;
    const long long n = (long long)B * (((long long)T + GL_NCOLS - 1) / GL_NCOLS) * C;
    return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int alm_gate_loop_norm_bwd(const float* dxn, const float* x, const float* gamma, const float* g, float* dx, float* dgamma, float* ws,
                                      long long ws_floats, int B, int C, int T, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0 || !dxn || !x || !gamma || !g || !dx || !dgamma || !ws) return ALM_ERR_BAD_ARG;
    const int need = alm_gate_loop_norm_bwd_ws_floats(B, C, T);
    if (need < 0 || B > 65535) return ALM_ERR_UNSUPPORTED;
    if (ws_floats < need) return ALM_ERR_BAD_ARG;
    const int nbx = (int)(((long long)T + GL_NCOLS - 1) / GL_NCOLS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gl_norm_bwd_kernel, dim3((unsigned)nbx, (unsigned)B), dim3(256), 0, st, dxn, x, gamma, g, dx, ws, C, T);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(gl_dgamma_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, (const float*)ws, dgamma, C, B * nbx);
    ALM_LAUNCH_CHECK();
    return 0;
}
