// Windowed-sinc polyphase resampling (soundstream.py:779-795 process_input -> torchaudio.functional.resample; third-party, restated in
// audiolm-pytorch_amd/resample.py), fp32, forward and adjoint.
//
// Both directions are one polyphase correlation: out[f * nph + ph] = sum_k tap(ph, k) * in_pad[f * stride + k], k < taps, where
// in_pad[i] = in[i - lpad] inside [0, len_in) and 0 outside (the zero padding is done while staging: no padded copy, no memset).
//   forward : stride = o, nph = n, taps = T = 2W + o, lpad = W,     tap(p, k) = K[p][k]
//   adjoint : stride = n, nph = o, taps = D n,        lpad = dmax n, tap(u, m) = K[p][d o + u + W] (0 outside [0, T)),
//             d = dmax - m / n, p = m % n, dmax = (W + o - 1) / o, D = 2 dmax + 1
// The adjoint follows from substituting dx index i = s o + u and d = s - j into dx[i] = sum_{j,p} K[p][i + W - j o] dy[j n + p]: a gather over
// the frames whose taps cover i (no atomics, bitwise deterministic).  Every tap is computed, near-zero ones included.
//
// Workgroup = 256 threads = one tile of J frames x PT phases of one row (rows strided by gridDim.y).  Thread = PR consecutive phases x JR frames
// (register blocking: one table read serves JR frames, one input read serves PR phases).  The input window of the tile ((J - 1) stride + taps
// samples) is staged in LDS once with coalesced loads; the table is staged in LDS k-major ([taps][PTp]: the PR phases of a thread are one
// ds_read_b128) when it fits RS_TABLE_LDS_BUDGET, else read from global memory, where it stays L2-resident.  The outputs go through LDS
// (aliasing the input window) and leave as J rows of PT contiguous floats: coalesced plain vector stores.
#include "common.hpp"
#include "launch.hpp"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_JR = 8;                                    // frames per thread
constexpr size_t RS_TABLE_LDS_BUDGET = 64 * 1024;           // bytes of staged table per workgroup
constexpr size_t RS_LDS_MAX = 160 * 1024;

struct RsArgs {
    const float* in;
    long long ld_in;
    float* out;
    long long ld_out;
    const float* K;               // [n][T]
    long long rows, len_in, len_out, frames, lpad;
    int stride, nph, taps;
    int PT, PTp, NPB, FS, J, nptiles;
    int o, n, T, W, dmax;         // geometry of K (the adjoint derives its taps from it)
};

template <bool ADJ>
__device__ __forceinline__ float rs_tap(const RsArgs& a, int ph, int k) {
    if (!ADJ) return a.K[(long long)ph * a.T + k];
    const int q = k / a.n;
    const int p = k - q * a.n;
    const int c = (a.dmax - q) * a.o + ph + a.W;
    return (c >= 0 && c < a.T) ? a.K[(long long)p * a.T + c] : 0.f;
}

template <int PR, bool TLDS, bool ADJ>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    const int tid = threadIdx.x;
    const int ptile = (int)(blockIdx.x % (unsigned)a.nptiles);
    const long long f0 = (long long)(blockIdx.x / (unsigned)a.nptiles) * a.J;
    const int p0 = ptile * a.PT;
    const int PTt = min(a.PT, a.nph - p0);                 // phases of this tile
    const int PTp = a.PTp, taps = a.taps, stride = a.stride;
    float* Ks = rs_smem;
    float* xs = rs_smem + (TLDS ? (long long)taps * PTp : 0);

    if (TLDS) {
        for (int q = tid; q < taps * PTp; q += RS_THREADS) {
            const int pl = q / taps, k = q - pl * taps;
            Ks[k * PTp + pl] = pl < PTt ? rs_tap<ADJ>(a, p0 + pl, k) : 0.f;
        }
    }
    const int pb = tid % a.NPB, fs = tid / a.NPB;
    const bool active = fs < a.FS;
    const int Lw = (a.J - 1) * stride + taps;
    const int fstep = a.FS * stride;

    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        const float* x = a.in + row * a.ld_in;
        const long long base = f0 * stride - a.lpad;
        for (int m = tid; m < Lw; m += RS_THREADS) {
            const long long g = base + m;
            xs[m] = (g >= 0 && g < a.len_in) ? x[g] : 0.f;
        }
        __syncthreads();

        float acc[RS_JR][PR];
#pragma unroll
        for (int r = 0; r < RS_JR; ++r)
#pragma unroll
            for (int i = 0; i < PR; ++i) acc[r][i] = 0.f;
        if (active) {
            const float* xr = xs + fs * stride;
#pragma unroll 2
            for (int k = 0; k < taps; ++k) {
                float kv[PR];
                if (TLDS) {
                    if (PR == 4) {
                        const float4 v = *reinterpret_cast<const float4*>(Ks + k * PTp + pb * 4);
                        kv[0] = v.x; kv[1] = v.y; kv[2] = v.z; kv[3] = v.w;
                    } else {
                        kv[0] = Ks[k * PTp + pb * PR];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < PR; ++i) {
                        const int pl = pb * PR + i;
                        kv[i] = pl < PTt ? rs_tap<ADJ>(a, p0 + pl, k) : 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < RS_JR; ++r) {
                    const float xv = xr[r * fstep + k];
#pragma unroll
                    for (int i = 0; i < PR; ++i) acc[r][i] = fmaf(kv[i], xv, acc[r][i]);
                }
            }
        }
        __syncthreads();                                    // every read of the window is done: the outputs reuse its LDS
        if (active) {
#pragma unroll
            for (int r = 0; r < RS_JR; ++r)
#pragma unroll
                for (int i = 0; i < PR; ++i) {
                    const int pl = pb * PR + i;
                    if (pl < PTt) xs[(fs + r * a.FS) * PTt + pl] = acc[r][i];
                }
        }
        __syncthreads();
        float* y = a.out + row * a.ld_out;
        for (int q = tid; q < a.J * PTt; q += RS_THREADS) {
            const int fl = q / PTt, pl = q - fl * PTt;
            const long long f = f0 + fl;
            const long long idx = f * a.nph + p0 + pl;
            if (f < a.frames && idx < a.len_out) y[idx] = xs[q];
        }
        __syncthreads();                                    // the next row overwrites the window
    }
}

template <int PR, bool TLDS, bool ADJ>
int rs_launch(const RsArgs& a, unsigned gx, unsigned gy, size_t lds, hipStream_t st) {
    const int rc = alm_lds_limit(reinterpret_cast<const void*>(resample_kernel<PR, TLDS, ADJ>), (int)RS_LDS_MAX);
    if (rc) return rc;
    hipLaunchKernelGGL((resample_kernel<PR, TLDS, ADJ>), dim3(gx, gy), dim3(RS_THREADS), lds, st, a);
    ALM_LAUNCH_CHECK();
    return 0;
}

template <bool ADJ>
int rs_run(RsArgs a, void* stream) {
    const int PR = a.nph >= 3 ? 4 : 1;
    a.PT = a.nph < 128 * PR ? a.nph : 128 * PR;            // <= 128 phase blocks: at least 2 frame slots per workgroup
    a.NPB = (a.PT + PR - 1) / PR;
    a.PTp = a.NPB * PR;
    a.nptiles = (a.nph + a.PT - 1) / a.PT;
    bool tlds = (size_t)a.taps * a.PTp * sizeof(float) <= RS_TABLE_LDS_BUDGET;
    int FS = RS_THREADS / a.NPB;
    size_t lds = 0;
    for (;;) {
        const long long J = (long long)FS * RS_JR;
        const long long win = (J - 1) * a.stride + a.taps;
        const long long need = (tlds ? (long long)a.taps * a.PTp : 0) + (win > J * a.PT ? win : J * a.PT);
        if (need * (long long)sizeof(float) <= (long long)RS_LDS_MAX) {
            lds = (size_t)need * sizeof(float);
            break;
        }
        if (FS > 1) FS = FS / 2;
        else if (tlds) { tlds = false; FS = RS_THREADS / a.NPB; }
        else return ALM_ERR_UNSUPPORTED;                    // one 8-frame window exceeds the LDS (o in the tens of thousands)
    }
    a.FS = FS;
    a.J = FS * RS_JR;
    const long long ftiles = (a.frames + a.J - 1) / a.J;
    if (ftiles * a.nptiles > 0x7fffffffLL) return ALM_ERR_UNSUPPORTED;
    const unsigned gx = (unsigned)(ftiles * a.nptiles);
    const unsigned gy = (unsigned)(a.rows < 65535 ? a.rows : 65535);
    hipStream_t st = (hipStream_t)stream;
    if (PR == 4) return tlds ? rs_launch<4, true, ADJ>(a, gx, gy, lds, st) : rs_launch<4, false, ADJ>(a, gx, gy, lds, st);
    return tlds ? rs_launch<1, true, ADJ>(a, gx, gy, lds, st) : rs_launch<1, false, ADJ>(a, gx, gy, lds, st);
}

// shared argument contract of both entry points; 1 = nothing to do, 0 = launch, ALM_ERR_BAD_ARG
int rs_check(const void* in, long long ld_in, const void* out, long long ld_out, const float* table, int taps, long long rows, long long len_in,
             long long len_out, int o, int n, int W, long long in_len, long long out_len) {
    if (rows < 0 || len_in < 0 || len_out < 0 || o <= 0 || n <= 0 || W < 0 || taps != 2 * W + o) return ALM_ERR_BAD_ARG;
    if (len_in > (1LL << 62) / n) return ALM_ERR_BAD_ARG;
    if (len_out != (len_in * n + o - 1) / o) return ALM_ERR_BAD_ARG;
    if ((long long)n * taps > 0x7fffffffLL) return ALM_ERR_BAD_ARG;
    if (rows == 0 || out_len == 0) return 1;
    if (!in || !out || !table || ld_in < in_len || ld_out < out_len) return ALM_ERR_BAD_ARG;
    return 0;
}

}  // namespace

extern "C" int alm_resample_sinc(const float* x, long long ld_x, float* y, long long ld_y, const float* table, int taps, long long rows,
                                 long long len_in, long long len_out, int o, int n, int W, void* stream) {
    const int c = rs_check(x, ld_x, y, ld_y, table, taps, rows, len_in, len_out, o, n, W, len_in, len_out);
    if (c != 0) return c == 1 ? 0 : c;
    RsArgs a{};
    a.in = x; a.ld_in = ld_x; a.out = y; a.ld_out = ld_y; a.K = table;
    a.rows = rows; a.len_in = len_in; a.len_out = len_out; a.frames = (len_out + n - 1) / n; a.lpad = W;
    a.stride = o; a.nph = n; a.taps = taps;
    a.o = o; a.n = n; a.T = taps; a.W = W; a.dmax = 0;
    return rs_run<false>(a, stream);
}

extern "C" int alm_resample_sinc_bwd(const float* dy, long long ld_dy, float* dx, long long ld_dx, const float* table, int taps, long long rows,
                                     long long len_in, long long len_out, int o, int n, int W, void* stream) {
    const int c = rs_check(dy, ld_dy, dx, ld_dx, table, taps, rows, len_in, len_out, o, n, W, len_out, len_in);
    if (c != 0) return c == 1 ? 0 : c;
    const int dmax = (W + o - 1) / o;
    if ((long long)(2 * dmax + 1) * n > 0x7fffffffLL) return ALM_ERR_BAD_ARG;
    RsArgs a{};
    a.in = dy; a.ld_in = ld_dy; a.out = dx; a.ld_out = ld_dx; a.K = table;
    a.rows = rows; a.len_in = len_out; a.len_out = len_in; a.frames = (len_in + o - 1) / o; a.lpad = (long long)dmax * n;
    a.stride = n; a.nph = o; a.taps = (2 * dmax + 1) * n;
    a.o = o; a.n = n; a.T = taps; a.W = W; a.dmax = dmax;
    return rs_run<true>(a, stream);
}
