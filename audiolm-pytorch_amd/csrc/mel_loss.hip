// Multi-spectral mel-spectrogram reconstruction loss of SoundStream training (reference soundstream.py:645-672, :933-945; eq. (4) / (5) of the
// SoundStream paper), fp32.  torchaudio.transforms.MelSpectrogram (power 2, centred reflect padding, one-sided, HTK filterbank) per scale, then per
// frame the L1 norm of the mel difference and the L2 norm of the log-mel difference, averaged over frames.  No atomics: every sum has one fixed order.
//
// Every matrix product is gemm64_kernel of gemm64.hpp (the exact-fp32 matrix core) with its own functor; real and fake waves run as ONE batch
// [real | fake] of B = 2 Bh rows.
//   power spectrum  : the DFT product of the STFT (M = 2 F rows (f, re | im), N = B T, A = the windowed DFT basis [n_fft][2 F], B = the frame sample
//                     with the reflect padding as index mirroring) whose epilogue takes rows 2 f and 2 f + 1 of a column together (store2) and writes
//                     P [B][F][T] = re^2 + im^2; the complex value itself is written only for the rows from `x_from` on (the fake half: the backward
//                     needs it, dX = 2 X dP).  The reduction runs over [k_lo, k_hi), the support of the window inside n_fft: the basis rows outside
//                     are exact zeros.  `normalized` (torchaudio's "window" normalisation, 1 / sqrt(sum w^2)) is inside the basis.
//   mel projection  : Mel [B][n_mels][T] = fb^T P, M = n_mels, N = B T, K = F; fb [F][n_mels] in torchaudio's layout.
//   per-frame loss  : one thread per frame (b, t) of the first half walks the n_mels column of both halves: l1 = sum |Mo - Mr|,
//                     l2 = sqrt(sum (log max(Mo, eps) - log max(Mr, eps))^2), eps = 1e-20; l2 is kept per frame for the backward.  Each block sums a
//                     contiguous span of frames in a fixed lane order; a second one-block kernel adds the blocks' parts in index order and writes
//                     means = (mean l1, mean l2) and loss = mean l1 + alpha mean l2.
//   backward        : dMel of the fake half, elementwise: -g / (Bh T) sign(Mo - Mr) - g alpha / (Bh T) (log Mo - log Mr) / l2 [Mr >= eps] / Mr, with
//                     torch's conventions: sign(0) = 0, nothing through an inactive clamp, nothing where l2 = 0 (each an exact 0, never 0 * inf).
//                     Then dP = fb dMel (M = F, N = Bh T, K = n_mels) whose epilogue writes dX = 2 X dP; alm_stft_bwd takes dX to the wave.
#include "gemm64.hpp"

namespace {

constexpr int RED_MAX_BLOCKS = 1024;
constexpr float MEL_EPS = 1e-20f;
constexpr long long I31 = 0x7fffffffLL;

struct MelPowerOp {
    const float* x; const float* basis; float* P; float* X;
    int M, N, klo, khi, len, hop, pad, F, T, x_from;
    struct NState { int b, t, base; };
    __device__ int k_lo(int) const { return klo; }
    __device__ int k_hi(int) const { return khi; }
    __device__ void decode_n(int n, NState& s) const { s.b = n / T; s.t = n - s.b * T; s.base = s.t * hop - pad; }
    __device__ float a(int m, int k) const { return basis[(size_t)k * M + m]; }
    __device__ float b(int k, const NState& s) const {
        int pos = s.base + k;
        if (pos < 0) pos = -pos;
        if (pos >= len) pos = 2 * (len - 1) - pos;                // len > n_fft / 2: one reflection lands inside
        return x[(size_t)s.b * len + pos];
    }
    __device__ void store2(int m, const NState& s, float re, float im, int) const {       // m even: (re, im) of frequency m / 2
        const int f = m >> 1;
        P[((size_t)s.b * F + f) * T + s.t] = re * re + im * im;
        if (X != nullptr && s.b >= x_from) reinterpret_cast<float2*>(X)[((size_t)(s.b - x_from) * F + f) * T + s.t] = make_float2(re, im);
    }
};

struct MelProjectOp {                                             // Mel [B][n_mels][T] = fb^T [n_mels][F] x P [F][B T]
    const float* P; const float* fb; float* mel;
    int M, N, K, T;
    struct NState { size_t in, out; };
    __device__ int k_lo(int) const { return 0; }
    __device__ int k_hi(int) const { return K; }
    __device__ void decode_n(int n, NState& s) const {
        const int b = n / T, t = n - b * T;
        s.in = (size_t)b * K * T + t, s.out = (size_t)b * M * T + t;
    }
    __device__ float a(int m, int k) const { return fb[(size_t)k * M + m]; }
    __device__ float b(int k, const NState& s) const { return P[s.in + (size_t)k * T]; }
    __device__ void store(int m, const NState& s, float v, int) const { mel[s.out + (size_t)m * T] = v; }
};

struct MelPowerBwdOp {                                            // dP [F][Bh T] = fb [F][n_mels] x dMel [n_mels][Bh T]; written as dX = 2 X dP
    const float* dmel; const float* fb; const float* X; float* dX;
    int M, N, K, T;
    struct NState { size_t in, out; };
    __device__ int k_lo(int) const { return 0; }
    __device__ int k_hi(int) const { return K; }
    __device__ void decode_n(int n, NState& s) const {
        const int b = n / T, t = n - b * T;
        s.in = (size_t)b * K * T + t, s.out = (size_t)b * M * T + t;
    }
    __device__ float a(int m, int k) const { return fb[(size_t)m * K + k]; }
    __device__ float b(int k, const NState& s) const { return dmel[s.in + (size_t)k * T]; }
    __device__ void store(int m, const NState& s, float v, int) const {
        const size_t o = s.out + (size_t)m * T;
        const float2 xv = reinterpret_cast<const float2*>(X)[o];
        reinterpret_cast<float2*>(dX)[o] = make_float2(2.f * xv.x * v, 2.f * xv.y * v);
    }
};

// mel [2 Bh][n_mels][T]; frames [lo, hi) of this block, thread per frame; norms [Bh T]; part[blockIdx.x] = sum l1, part[RED_MAX_BLOCKS + blockIdx.x] = sum l2
__global__ __launch_bounds__(256) void mel_frame_loss_kernel(const float* __restrict__ mel, float* __restrict__ norms, float* __restrict__ part, int Bh,
                                                             int n_mels, int T, int span) {
    const long long frames = (long long)Bh * T, lo = (long long)blockIdx.x * span, hi = min(frames, lo + span);
    const size_t half = (size_t)Bh * n_mels * T;
    float s1 = 0.f, s2 = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const int b = (int)(i / T), t = (int)(i - (long long)b * T);
        const float* o = mel + (size_t)b * n_mels * T + t;
        float l1 = 0.f, sq = 0.f;
        for (int m = 0; m < n_mels; ++m) {
            const float mo = o[(size_t)m * T], mr = o[half + (size_t)m * T];
            l1 += fabsf(mo - mr);
            const float d = logf(fmaxf(mo, MEL_EPS)) - logf(fmaxf(mr, MEL_EPS));
            sq = fmaf(d, d, sq);
        }
        const float l2 = sqrtf(sq);
        norms[i] = l2;
        s1 += l1, s2 += l2;
    }
    s1 = block_sum(s1);
    s2 = block_sum(s2);
    if (threadIdx.x == 0) part[blockIdx.x] = s1, part[RED_MAX_BLOCKS + blockIdx.x] = s2;
}

__global__ __launch_bounds__(256) void mel_loss_finish_kernel(const float* __restrict__ part, float* __restrict__ loss, float* __restrict__ means, int nparts,
                                                              float inv_frames, float alpha) {
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s1 += part[i], s2 += part[RED_MAX_BLOCKS + i];
    s1 = block_sum(s1);
    s2 = block_sum(s2);
    if (threadIdx.x == 0) {
        const float m1 = s1 * inv_frames, m2 = s2 * inv_frames;
        means[0] = m1, means[1] = m2;
        loss[0] = m1 + alpha * m2;
    }
}

// dmel [Bh][n_mels][T] (the fake half), one thread per element; gout: the upstream gradient of the scale's loss, a scalar in device memory
__global__ __launch_bounds__(256) void mel_frame_loss_bwd_kernel(const float* __restrict__ mel, const float* __restrict__ norms, const float* __restrict__ gout,
                                                                 float* __restrict__ dmel, int n_mels, int T, long long half, float inv_frames, float alpha) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= half) return;
    const long long row = i / T;                                  // b n_mels + m
    const long long frame = (row / n_mels) * T + (i - row * T);
    const float g = gout[0] * inv_frames;
    const float mo = mel[i], mr = mel[half + i], d = mo - mr;
    float v = d > 0.f ? -g : d < 0.f ? g : 0.f;                   // sign(0) = 0
    const float l2 = norms[frame];
    if (l2 > 0.f && mr >= MEL_EPS) {                              // no gradient where the norm is 0 or the clamp holds the value
        const float ld = logf(fmaxf(mo, MEL_EPS)) - logf(mr);
        v -= g * alpha * (ld / l2) / mr;
    }
    dmel[i] = v;
}

// the envelope shared by the products over frames: every flattened GEMM index is 32-bit, tensor offsets are size_t
bool frames_fit(int B, int n, int n_fft, int hop, int T) {
    return T >= 1 && (long long)B * T + 64 < I31 && (long long)n + 2LL * n_fft < I31 && (long long)T * hop < I31;
}

int frame_span(long long frames) {
    long long span = 256;
    while ((frames + span - 1) / span > RED_MAX_BLOCKS) span *= 2;
    return span >= I31 ? -1 : (int)span;
}

}  // namespace

extern "C" int alm_mel_power_fwd(const float* x, const float* basis, float* P, float* X, int B, int x_from, int n, int n_fft, int hop, int F, int k_lo,
                                 int k_hi, void* stream) {
    if (B <= 0 || n <= 0 || n_fft <= 0 || hop <= 0 || F <= 0 || F > n_fft || x_from < 0 || x_from > B || k_lo < 0 || k_lo >= k_hi || k_hi > n_fft)
        return ALM_ERR_BAD_ARG;
    const int T = alm_stft_frames(n, n_fft, hop);
    if (T < 1 || !frames_fit(B, n, n_fft, hop, T) || (2LL * F + 63) / 64 > 65535) return ALM_ERR_UNSUPPORTED;
    MelPowerOp op = {x, basis, P, X, 2 * F, B * T, k_lo, k_hi, n, hop, n_fft / 2, F, T, x_from};
    return launch_gemm<MelPowerOp, true, false>(op, 1, (hipStream_t)stream);
}

extern "C" int alm_mel_project_fwd(const float* P, const float* fb, float* mel, int B, int F, int T, int n_mels, void* stream) {
    if (B <= 0 || F <= 0 || T <= 0 || n_mels <= 0) return ALM_ERR_BAD_ARG;
    if ((long long)B * T + 64 >= I31 || (long long)F + 64 >= I31 || (n_mels + 63LL) / 64 > 65535) return ALM_ERR_UNSUPPORTED;
    MelProjectOp op = {P, fb, mel, n_mels, B * T, F, T};
    return launch_gemm<MelProjectOp, true, false>(op, 1, (hipStream_t)stream);
}

extern "C" int alm_mel_loss_ws_floats(void) { return 2 * RED_MAX_BLOCKS; }

extern "C" int alm_mel_frame_loss_fwd(const float* mel, float* norms, float* loss, float* means, float* ws, int Bh, int n_mels, int T, float alpha,
                                      void* stream) {
    if (Bh <= 0 || n_mels <= 0 || T <= 0 || norms == nullptr || loss == nullptr || means == nullptr || ws == nullptr) return ALM_ERR_BAD_ARG;
    const long long frames = (long long)Bh * T;
    const int span = frame_span(frames);
    if (frames >= I31 || span < 0) return ALM_ERR_UNSUPPORTED;
    const int nparts = (int)((frames + span - 1) / span);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mel_frame_loss_kernel, dim3(nparts), dim3(256), 0, st, mel, norms, ws, Bh, n_mels, T, span);
    ALM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mel_loss_finish_kernel, dim3(1), dim3(256), 0, st, ws, loss, means, nparts, (float)(1.0 / (double)frames), alpha);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_mel_frame_loss_bwd(const float* mel, const float* norms, const float* gout, float* dmel, int Bh, int n_mels, int T, float alpha,
                                      void* stream) {
    if (Bh <= 0 || n_mels <= 0 || T <= 0 || gout == nullptr) return ALM_ERR_BAD_ARG;
    const long long frames = (long long)Bh * T, half = frames * n_mels;
    if (frames >= I31 || (half + 255) / 256 >= I31) return ALM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mel_frame_loss_bwd_kernel, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mel, norms, gout, dmel, n_mels, T,
                       half, (float)(1.0 / (double)frames), alpha);
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_mel_power_bwd(const float* dmel, const float* fb, const float* X, float* dX, int B, int F, int T, int n_mels, void* stream) {
    if (B <= 0 || F <= 0 || T <= 0 || n_mels <= 0) return ALM_ERR_BAD_ARG;
    if ((long long)B * T + 64 >= I31 || (long long)n_mels + 64 >= I31 || (F + 63LL) / 64 > 65535) return ALM_ERR_UNSUPPORTED;
    MelPowerBwdOp op = {dmel, fb, X, dX, F, B * T, n_mels, T};
    return launch_gemm<MelPowerBwdOp, false, false>(op, 1, (hipStream_t)stream);
}
