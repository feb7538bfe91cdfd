// EnCodec 24 kHz (causal SEANet + LSTM + residual VQ; reference encodec.py:25-177 wraps Meta's model) on gfx950, fp32 throughout: the codes are an
// argmin over float distances, so every matrix product runs on the exact-fp32 matrix core or in fp32 fma chains.  The residual VQ is csrc/codec.hip's.
//
//   conv1d_causal_pre : the SoundStream causal conv (csrc/conv1d.hpp) with a PRE-activation flag.  SEANet puts the ELU before each conv; where a tensor
//                       is needed both raw (the 1x1 shortcut of a residual block, the residual add) and through the ELU (the k = 3 conv, the strided
//                       conv that follows the block), the ELU is applied to the activation operand on its way to the MFMA instead of being stored.
//   lstm_step         : nn.LSTM(H, H, L) over time, gate order i f g o, zero initial state.  ONE launch per time step, all of them issued by one C
//                       call.  In launch t, blockIdx.y = l advances layer l to time t - l (T + L - 1 launches), so layer l reads what layer l - 1
//                       wrote one launch earlier and what it wrote itself one launch earlier: the launch boundary is the only synchronisation.  No
//                       workgroup waits for another one -- no grid barrier, no flags, no spinning, no cooperative launch.
//                       A wave owns ONE hidden unit: its four gate rows of W_hh (and W_ih for l > 0) are read once per step, coalesced, and multiplied
//                       with h_{t-1} (and the layer below's h_t) of 8 batch rows staged in LDS (<= 64 KB; more rows loop in chunks of 8).  Lane j takes
//                       k = j, j + 64, ...; the 4 x 8 partial sums are reduced across the lanes by xor butterflies (a fixed order: runs are bitwise
//                       repeatable and a batch row does not depend on its neighbours); lane b then applies the cell update of batch row b.
//                       Layer 0's input projection for all steps is a GEMM the caller runs beforehand (xproj [T][B][4H]: each step reads contiguous
//                       rows).  c lives in a [L][B][H] buffer that only the owning wave touches.
#include "common.hpp"
#include "conv1d.hpp"

namespace {

constexpr int LSTM_BC = 8;            // batch rows per LDS chunk
constexpr int LSTM_WAVES = 4;         // hidden units per workgroup

struct LstmArgs {
    const float* xproj;               // [T][B][4H]   W_ih_l0 x_t (no bias)
    const float* w_ih;                // [L][4H][H]   (layer 0's slice is not read)
    const float* w_hh;                // [L][4H][H]
    const float* bias;                // [L][4H]      b_ih + b_hh
    float* hseq;                      // [L][T][B][H]
    float* c;                         // [L][B][H]
    const float* skip;                // [T][B][H] or NULL
    float* out;                       // [B][H][T] or NULL: last layer's h (+ skip)
    int T, B, H, L, t;
};

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

__global__ __launch_bounds__(64 * LSTM_WAVES) void lstm_step_kernel(LstmArgs a) {
    extern __shared__ float vec[];                                 // [LSTM_BC][K]: h_{t-1} of this layer | h_t of the layer below
    const int l = blockIdx.y, tt = a.t - l;
    if (tt < 0 || tt >= a.T) return;                               // uniform over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, B = a.B;
    const int K = l > 0 ? 2 * H : H;
    const int u = blockIdx.x * LSTM_WAVES + wave;
    const bool unit_ok = u < H;
    const float* hprev = tt > 0 ? a.hseq + ((long long)l * a.T + tt - 1) * B * H : nullptr;
    const float* below = l > 0 ? a.hseq + ((long long)(l - 1) * a.T + tt) * B * H : nullptr;
    const float* whh = a.w_hh + (long long)l * 4 * H * H;
    const float* wih = a.w_ih + (long long)l * 4 * H * H;

    for (int b0 = 0; b0 < B; b0 += LSTM_BC) {
        const int nb = min(LSTM_BC, B - b0);
        for (int i = threadIdx.x; i < LSTM_BC * K; i += 64 * LSTM_WAVES) {
            const int b = i / K, k = i - b * K;
            float v = 0.f;
            if (b < nb) {
                if (k < H) v = hprev ? hprev[(long long)(b0 + b) * H + k] : 0.f;
                else v = below[(long long)(b0 + b) * H + (k - H)];
            }
            vec[i] = v;
        }
        __syncthreads();
        if (unit_ok) {
            float acc[4][LSTM_BC];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int b = 0; b < LSTM_BC; ++b) acc[g][b] = 0.f;
            if (tt > 0) {                                          // h_{-1} = 0: nothing to add at the first step
                for (int k = lane; k < H; k += 64) {
                    float w[4], h[LSTM_BC];
#pragma unroll
                    for (int g = 0; g < 4; ++g) w[g] = whh[((long long)g * H + u) * H + k];
#pragma unroll
                    for (int b = 0; b < LSTM_BC; ++b) h[b] = vec[b * K + k];
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int b = 0; b < LSTM_BC; ++b) acc[g][b] = fmaf(w[g], h[b], acc[g][b]);
                }
            }
            if (l > 0) {
                for (int k = lane; k < H; k += 64) {
                    float w[4], h[LSTM_BC];
#pragma unroll
                    for (int g = 0; g < 4; ++g) w[g] = wih[((long long)g * H + u) * H + k];
#pragma unroll
                    for (int b = 0; b < LSTM_BC; ++b) h[b] = vec[b * K + H + k];
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int b = 0; b < LSTM_BC; ++b) acc[g][b] = fmaf(w[g], h[b], acc[g][b]);
                }
            }
            float pre[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int b = 0; b < LSTM_BC; ++b) {
                    const float s = wave_sum(acc[g][b]);           // every lane holds the sum
                    if (lane == b) pre[g] = s;
                }
            if (lane < nb) {
                const int bb = b0 + lane;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    pre[g] += a.bias[((long long)l * 4 + g) * H + u];
                    if (l == 0) pre[g] += a.xproj[((long long)tt * B + bb) * 4 * H + g * H + u];
                }
                const long long ci = ((long long)l * B + bb) * H + u;
                const float cold = tt > 0 ? a.c[ci] : 0.f;
                const float cnew = sigmoid_f(pre[1]) * cold + sigmoid_f(pre[0]) * tanhf(pre[2]);
                const float h = sigmoid_f(pre[3]) * tanhf(cnew);
                a.c[ci] = cnew;
                a.hseq[(((long long)l * a.T + tt) * B + bb) * H + u] = h;
                if (l == a.L - 1 && a.out)
                    a.out[((long long)bb * H + u) * a.T + tt] = a.skip ? h + a.skip[((long long)tt * B + bb) * H + u] : h;
            }
        }
        __syncthreads();                                           // the next chunk overwrites vec
    }
}

}  // namespace

// alm_conv1d_causal with a pre-activation: out = act(bias + conv(pre_elu ? ELU(x) : x)) (+ residual); same packing, padding and limits
extern "C" int alm_conv1d_causal_pre(const float* x, const float* wp, const float* bias, const float* residual, float* out, int B, int Cin, int Cout,
                                     int Tin, int ksize, int stride, int dilation, int pre_elu, int elu, int zero_pad, void* stream) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Tin <= 0 || ksize <= 0 || stride <= 0 || dilation <= 0) return ALM_ERR_BAD_ARG;
    const int pad = dilation * (ksize - 1) + 1 - stride;
    if (pad < 0 || (!zero_pad && pad >= Tin) || Tin < stride || B > 65535) return ALM_ERR_UNSUPPORTED;      // zero pad: nothing is reflected, one frame is enough
    if ((long long)(Cout + 32) * Tin * 4 >= 0x7fffffffLL || (long long)(Cin + 2) * Tin * 4 >= 0x7fffffffLL ||
        (long long)ksize * (Cin + 1) * (Cout + 31) * 4 >= 0x7fffffffLL)
        return ALM_ERR_UNSUPPORTED;                                // 32-bit buffer offsets
    const int Tout = (Tin - stride) / stride + 1;
    ConvArgs a{x, wp, bias, residual, out, B, Cin, (Cin + 1) & ~1, Cout, (Cout + 31) & ~31, Tin, Tout, ksize, stride, dilation, pad, elu, zero_pad};
    const int gx = (Tout + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    const bool wide = a.CoutP % 64 == 0;
    const dim3 grid(gx, a.CoutP / (wide ? 64 : 32), B);
    if (pre_elu) {
        if (wide) hipLaunchKernelGGL((conv1d_causal_kernel<2, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv1d_causal_kernel<1, true>), grid, dim3(256), 0, st, a);
    } else {
        if (wide) hipLaunchKernelGGL((conv1d_causal_kernel<2, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv1d_causal_kernel<1, false>), grid, dim3(256), 0, st, a);
    }
    ALM_LAUNCH_CHECK();
    return 0;
}

extern "C" int alm_lstm_launches(int T, int L) { return T > 0 && L > 0 ? T + L - 1 : 0; }

// nn.LSTM(H, H, L) over T steps of B rows; see the header comment for the buffers.  skip / out may be NULL (out: [B][H][T] = h of the last layer + skip).
// H <= 1024 (the LDS chunk of 8 rows x 2 H floats), else ALM_ERR_UNSUPPORTED.
extern "C" int alm_lstm_seq(const float* xproj, const float* w_ih, const float* w_hh, const float* bias, float* hseq, float* c, const float* skip,
                            float* out, int T, int B, int H, int L, void* stream) {
    if (T <= 0 || B <= 0 || H <= 0 || L <= 0) return ALM_ERR_BAD_ARG;
    const size_t smem = (size_t)LSTM_BC * (L > 1 ? 2 : 1) * H * sizeof(float);
    if (smem > 64 * 1024 || L > 65535) return ALM_ERR_UNSUPPORTED;
    LstmArgs a{xproj, w_ih, w_hh, bias, hseq, c, skip, out, T, B, H, L, 0};
    const dim3 grid((H + LSTM_WAVES - 1) / LSTM_WAVES, L);
    const int n = alm_lstm_launches(T, L);
    for (int t = 0; t < n; ++t) {
        a.t = t;
        hipLaunchKernelGGL(lstm_step_kernel, grid, dim3(64 * LSTM_WAVES), smem, (hipStream_t)stream, a);
    }
    ALM_LAUNCH_CHECK();
    return 0;
}
