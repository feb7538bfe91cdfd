#!/usr/bin/env python
"""Kernel micro-benchmarks on the MI355X for the hot-path shapes (B=8 x N=2048 tokens, D=1024): every GEMM variant vs the vendor
BLAS yardstick (torch.matmul; NOT part of the product), attention fwd/bwd, hyper-connection kernels.  Prints one line per case:
name, ms, TFLOP/s or GB/s.   usage: python scripts/kbench.py [gemm] [attn] [hc] [misc] [t5] [convs_bwd] [local_attn_bwd] [rvq_train] [discr] [stft_discr] [mel_loss] [grad_penalty] [se_film] [fsq] [lfq] [gate_loop] [vqw2v]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audiolm_pytorch_amd as A  # noqa: E402,F401
from audiolm_pytorch_amd import ops, _lib  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
dev = torch.device('cuda:0')


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rnd(*shape, dtype=BF16):
    return (torch.rand(*shape, device=dev) * 2 - 1).to(dtype)


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def bench_gemm():
    T = 16384
    shapes = [('W1 fwd', T, 5472, 1024), ('W2 fwd', T, 1024, 2736), ('dHN dgrad', T, 2736, 1024), ('dXN2 dgrad', T, 1024, 5472),
              ('Wq fwd', T, 512, 1024), ('Wo fwd', T, 1024, 512), ('dAO dgrad', T, 512, 1024), ('dXN dgrad', T, 1024, 512), ('Wkv fwd', T, 128, 1024),
              ('dXkv dgrad', T, 1024, 128), ('square 4096', 4096, 4096, 4096)]
    print('--- NT GEMMs  C[M,N] = A[M,K] B[N,K]^T (bf16 out)')
    for name, M, N, K in shapes:
        Am, Bm = rnd(M, K), rnd(N, K)
        C = torch.empty((M, N), dtype=BF16, device=dev)
        fl = 2.0 * M * N * K
        ref = None
        line = f'{name:14s} {M}x{N}x{K}:'
        t = timeit(lambda: torch.matmul(Am, Bm.t(), out=C))
        ref = C.clone()
        line += f'  blas {t:.3f} ms {fl / t / 1e9:7.0f} TF |'
        for tile in (1, 2, 13, 11):
            if tile >= 2 and (M < 256 or N < 256):
                continue
            C.zero_()
            t = timeit(lambda: ops.gemm_nt_tile(Am, Bm, C, tile))
            line += f'  tile{tile} {t:.3f} ms {fl / t / 1e9:7.0f} TF (err {relerr(C, ref):.1e}) |'
        print(line, flush=True)
    print('--- TN split-K wgrads  C[M,N] = At[K,M]^T Bt[K,N] (fp32 out)')
    for name, M, N, K in [('dW1 half', 2730, 1024, T), ('dW2', 1024, 2730, T), ('dWq', 512, 1024, T), ('dWo', 1024, 512, T), ('dWkv', 128, 1024, T),
                          ('dWhead', 1025, 1024, 4096)]:
        At, Bt = rnd(K, (M + 7) // 8 * 8)[:, :M], rnd(K, (N + 7) // 8 * 8)[:, :N]
        C = torch.empty((M, N), dtype=F32, device=dev)
        fl = 2.0 * M * N * K
        t0 = timeit(lambda: torch.matmul(At.t(), Bt))
        ref = torch.matmul(At.t().float(), Bt.float())
        t = timeit(lambda: ops.gemm_tn_splitk(At, Bt, C))
        print(f'{name:14s} {M}x{N}x{K}:  blas {t0:.3f} ms {fl / t0 / 1e9:7.0f} TF |  tn-splitk {t:.3f} ms {fl / t / 1e9:7.0f} TF (err {relerr(C, ref):.1e}, '
              f'slices {_lib.query("alm_gemm_splitk_slices", M, N, K, 1)})', flush=True)


def bench_tn():
    """split-K plan / rasterisation sweep for the two big weight-gradient shapes, on the bench-only library (tuning hook almlab_debug_splitk)."""
    import gemm_lab
    lab = gemm_lab.bind()
    T, I, Ip, D = 16384, 2730, 2736, 1024
    dU, XN2 = rnd(T, 2 * Ip), rnd(T, D)
    dW1 = torch.empty((2, I, D), dtype=F32, device=dev)
    dY2, HN = rnd(T, D), rnd(T, Ip)
    dW2 = torch.empty((D, I), dtype=F32, device=dev)
    ws = torch.empty(1 << 28, dtype=F32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def f1():
        assert lab.almlab_gemm_bf16_tn_splitk(dU.data_ptr(), XN2.data_ptr(), dW1.data_ptr(), ws.data_ptr(), I, D, T, 2 * Ip, D, D, 2, Ip, 0, I * D, 1.0, 0, st) == 0

    def f2():
        assert lab.almlab_gemm_bf16_tn_splitk(dY2.data_ptr(), HN.data_ptr(), dW2.data_ptr(), ws.data_ptr(), D, I, T, D, Ip, I, 1, 0, 0, 0, 1.0, 0, st) == 0
    fl1, fl2 = 2.0 * 2 * I * D * T, 2.0 * D * I * T
    for raster in (0, 1):
        for tile, sl in [(0, 0), (2, 2), (2, 5), (3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 6)]:
            lab.almlab_debug_splitk(tile, sl, raster)
            assert lab.almlab_gemm_splitk_ws_floats(I, D, T, 2) <= ws.numel() and lab.almlab_gemm_splitk_ws_floats(D, I, T, 1) <= ws.numel()
            t1, t2 = timeit(f1, iters=10), timeit(f2, iters=10)
            print(f'raster {raster} tile {tile} slices {sl}:  dW1(batched x2) {t1:.3f} ms {fl1 / t1 / 1e9:5.0f} TF | dW2 {t2:.3f} ms {fl2 / t2 / 1e9:5.0f} TF', flush=True)
    lab.almlab_debug_splitk(0, 0, 1)


def bench_wgrad():
    """every weight-gradient contraction of one layer (+ the coarse head) with the automatic split-K plan"""
    T, I, Ip, D, H, dh = 16384, 2730, 2736, 1024, 8, 64
    dU, XN2, dY, HN, AO, dQ, XN, dKV, X = rnd(T, 2 * Ip), rnd(T, D), rnd(T, D), rnd(T, Ip), rnd(T, H * dh), rnd(T, H * dh), rnd(T, D), rnd(T, 2 * dh), rnd(T, D)
    cases = [
        ('dW1 (x | gate batched)', lambda C: ops.gemm_tn_splitk(dU.view(T, 2, Ip).permute(1, 0, 2)[:, :, :I], XN2, C), (2, I, D), 2 * I, D, 2),
        ('dW2', lambda C: ops.gemm_tn_splitk(dY, HN[:, :I], C), (D, I), D, I, 1),
        ('dWo', lambda C: ops.gemm_tn_splitk(dY, AO, C), (D, H * dh), D, H * dh, 1),
        ('dWq', lambda C: ops.gemm_tn_splitk(dQ, XN, C), (H * dh, D), H * dh, D, 1),
        ('dWkv', lambda C: ops.gemm_tn_splitk(dKV, X, C), (2 * dh, D), 2 * dh, D, 1),
    ]
    tot = 0.0
    for name, fn, shape, M, N, nb in cases:
        C = torch.empty(shape, dtype=F32, device=dev)
        t = timeit(lambda: fn(C), iters=20)
        sl = _lib.query('alm_gemm_splitk_slices', M // nb, N, T, nb)
        fl = 2.0 * M * N * T
        tot += t
        print(f'{name:24s} [{M}x{N}] K={T}: slices {sl:2d}  {t * 1e3:7.1f} us  {fl / t / 1e9:5.0f} TF')
    print(f'one layer: {tot * 1e3:.1f} us -> x6 = {tot * 6:.2f} ms/step; at the NT-256 rate (866 TF) it would be {313e9 / 866e12 * 6e3:.2f} ms')


def bench_attn():
    B, N, H, dh = 8, 2048, 8, 64
    M = B * N
    Q, KV = rnd(M, H * dh), rnd(M, 2 * dh)
    K_, V_ = KV[:, :dh], KV[:, dh:]
    mask = (torch.rand(B, N, device=dev) > 0.15).to(torch.uint8)
    mask[:, 0] = 1
    fl_f = 4.0 * B * H * dh * N * (N + 1) / 2
    AO, LSE = ops.mqa_attn_fwd(Q, K_, V_, mask, B, N, H, dh)
    t = timeit(lambda: ops.mqa_attn_fwd(Q, K_, V_, mask, B, N, H, dh))
    print(f'attn fwd  B{B} N{N} H{H}: {t:.3f} ms  {fl_f / t / 1e9:.0f} TF (causal-exact flops)')
    dAO = rnd(M, H * dh)
    t = timeit(lambda: ops.mqa_attn_bwd(Q, K_, V_, mask, AO, LSE, dAO, B, N, H, dh))
    print(f'attn bwd  B{B} N{N} H{H}: {t:.3f} ms  {2.5 * fl_f / t / 1e9:.0f} TF (2.5 x fwd flops)')


def bench_hc_old():
    from audiolm_pytorch_amd import core
    B, S, N, D = 8, 4, 2048, 1024
    M = B * N
    R = torch.randn(B, S, N, D, device=dev)
    hc = dict(Bb=torch.ones(S, device=dev), Aa=torch.randn(S, S + 1, device=dev), Wa=torch.randn(D, S + 1, device=dev) * 0.02,
              sa=torch.tensor(0.01, device=dev), wb=torch.randn(D, device=dev) * 0.02, sb=torch.tensor(0.01, device=dev),
              gamma=torch.zeros(D, device=dev))
    lng = torch.ones(D, device=dev)
    Rb = R.numel() * 4
    X, XN, mean, rstd, coef = ops.hc_width_fwd(R, hc, lng, B, S, N, D, want_x=True)
    t = timeit(lambda: ops.hc_width_fwd(R, hc, lng, B, S, N, D, want_x=True))
    print(f'hc_width_fwd: {t:.3f} ms  {(Rb + 2 * M * D * 2) / t / 1e6:.0f} GB/s (alg bytes: read R, write X, XN)')
    Y = rnd(M, D)
    t = timeit(lambda: ops.hc_depth_fwd(R, Y, coef, B, S, N, D))
    print(f'hc_depth_fwd: {t:.3f} ms  {(2 * Rb + M * D * 2) / t / 1e6:.0f} GB/s (read R, Y; write R)')
    dR = torch.randn(B, S, N, D, device=dev)
    t = timeit(lambda: ops.hc_depth_bwd(dR, Y, coef, B, S, N, D))
    dY, dbeta = ops.hc_depth_bwd(dR, Y, coef, B, S, N, D)
    print(f'hc_depth_bwd: {t:.3f} ms  {(Rb + 2 * M * D * 2) / t / 1e6:.0f} GB/s (read dR, Y; write dY)')
    dX = torch.randn(M, D, device=dev)
    t = timeit(lambda: ops.hc_width_bwd(dR, dX, R, coef, dbeta, hc, B, S, N, D))
    print(f'hc_width_bwd: {t:.3f} ms  {(3 * Rb + M * D * 4) / t / 1e6:.0f} GB/s (read dR, R, dX; write dR)')


def bench_hc():
    B, S, N, D = 8, 4, 2048, 1024
    M = B * N
    R = torch.randn(B, S, N, D, device=dev)
    hc = dict(Bb=torch.ones(S, device=dev), Aa=torch.randn(S, S + 1, device=dev), Wa=torch.randn(D, S + 1, device=dev) * 0.02,
              sa=torch.tensor(0.01, device=dev), wb=torch.randn(D, device=dev) * 0.02, sb=torch.tensor(0.01, device=dev),
              gamma=torch.zeros(D, device=dev))
    lng = torch.ones(D, device=dev)
    Rb, Ab = R.numel() * 4, M * D * 2
    w = ops.hc_fwd(R, B, S, N, D, hc=hc, ln_gamma=lng)
    coef = w['coef']
    Y = rnd(M, D)
    for name, fn, byt in [
        ('hc fwd width only', lambda: ops.hc_fwd(R, B, S, N, D, hc=hc, ln_gamma=lng), Rb + 2 * Ab),
        ('hc fwd depth only', lambda: ops.hc_fwd(R, B, S, N, D, y_prev=Y, coef_prev=coef), 2 * Rb + Ab),
        ('hc fwd depth+width fused', lambda: ops.hc_fwd(R, B, S, N, D, y_prev=Y, coef_prev=coef, hc=hc, ln_gamma=lng), 2 * Rb + 3 * Ab),
        ('hc fwd final (depth+sum+LN)', lambda: ops.hc_fwd(R, B, S, N, D, y_prev=Y, coef_prev=coef, ln_gamma=lng, final=True), Rb + 2 * Ab + M * D * 4),
    ]:
        t = timeit(fn)
        print(f'{name:30s}: {t:.3f} ms  {byt / t / 1e6:.0f} GB/s algorithmic')
    dR = torch.randn(B, S, N, D, device=dev)
    dX = torch.randn(M, D, device=dev)
    dbeta = ops.hc_bwd(dR, B, S, N, D, y_prev=Y, coef_prev=coef)['dbeta']
    for name, fn, byt in [
        ('hc bwd depth only', lambda: ops.hc_bwd(dR, B, S, N, D, y_prev=Y, coef_prev=coef), Rb + 2 * Ab),
        ('hc bwd width only', lambda: ops.hc_bwd(dR, B, S, N, D, dx=dX, R=R, coef=coef, dbeta=dbeta, hc=hc), 3 * Rb + M * D * 4),
        ('hc bwd width+depth fused', lambda: ops.hc_bwd(dR, B, S, N, D, dx=dX, R=R, coef=coef, dbeta=dbeta, hc=hc, y_prev=Y, coef_prev=coef), 3 * Rb + M * D * 4 + 2 * Ab),
    ]:
        t = timeit(fn)
        print(f'{name:30s}: {t:.3f} ms  {byt / t / 1e6:.0f} GB/s algorithmic')


def bench_codec():
    """BASELINE configs[4] codec: SoundStream(codebook 4096, 8 quantizers, 24 kHz, strides 2*4*5*8) on 8 x 30 s of synthetic audio."""
    torch.manual_seed(0)
    ss = A.SoundStream(codebook_size=4096, rq_num_quantizers=8, target_sample_hz=24000, strides=(2, 4, 5, 8), use_local_attn=False)
    for r in ss.rq.rvqs:
        for q, l in enumerate(r.layers):
            l._codebook.embed.copy_(torch.randn(1, 4096, 512) * (0.5 ** q))
            l._codebook.initted.fill_(True)
    ss.to(dev)
    wave = torch.randn(8, 720000, device=dev) * 0.1
    x, _ = ss.process_input(wave)
    feats = ss.encode(x)
    t_enc = timeit(lambda: ss.encode(x), iters=3, warm=1)
    t_rvq = timeit(lambda: ss.rq(feats), iters=3, warm=1)
    t_all = timeit(lambda: ss.tokenize(wave), iters=3, warm=1)
    frames = feats.shape[0] * feats.shape[1]
    macs_enc = 8 * 720000 * 190.6e3
    macs_rvq = frames * 8 * 4096 * 512
    print(f'codec encoder   8 x 30 s @ 24 kHz: {t_enc:.2f} ms  {2 * macs_enc / t_enc / 1e9:.1f} TF fp32')
    print(f'codec rvq       {frames} frames x 8 x 4096 codes: {t_rvq:.2f} ms  {2 * macs_rvq / t_rvq / 1e9:.1f} TF fp32')
    print(f'codec tokenize  total {t_all:.2f} ms -> {frames * 8 / t_all * 1e3:.0f} codes/s, {8 * 30 / t_all * 1e3:.0f} x real time')


def bench_convs():
    """per-layer timing of the SoundStream encoder (8 x 30 s @ 24 kHz): every causal conv launch with its fp32 MFMA rate / HBM rate."""
    torch.manual_seed(0)
    ss = A.SoundStream(codebook_size=4096, rq_num_quantizers=8, target_sample_hz=24000, strides=(2, 4, 5, 8), use_local_attn=False).to(dev)
    from audiolm_pytorch_amd import soundstream as SS
    h = torch.randn(8, 1, 720000, device=dev) * 0.1
    rows = []

    def run(layer, x, **kw):
        y = layer.run(x, **kw)
        t = timeit(lambda: layer.run(x, **kw), iters=3, warm=1)
        cin, cout, k = layer.conv.in_channels, layer.conv.out_channels, layer.kernel_size
        fl = 2.0 * y.numel() * cin * k
        by = 4.0 * (x.numel() + y.numel() * (2 if kw.get('residual') is not None else 1))
        rows.append((f'{cin}->{cout} k{k} s{layer.stride} d{layer.dilation} T={x.shape[-1]}', t, fl / t / 1e9, by / t / 1e6))
        return y
    for layer in ss.encoder:
        if isinstance(layer, SS.CausalConv1d):
            h = run(layer, h)
        else:
            for sub in layer:
                if isinstance(sub, SS._ResidualFn):
                    a1 = run(sub.fn[0], h, elu=True)
                    h = run(sub.fn[2], a1, elu=True, residual=h)
                else:
                    h = run(sub, h)
    tot = sum(r[1] for r in rows)
    for name, t, tf, gb in rows:
        print(f'{name:40s} {t:7.3f} ms  {tf:6.1f} TF fp32  {gb:7.0f} GB/s')
    print(f'total {tot:.2f} ms')


def bench_convs_bwd():
    """backward kernels of the codec's conv stacks (csrc/codec_bwd.hip) at the config-5 encoder / decoder stage shapes (8 x 30 s @ 24 kHz): input
    gradient (reflect fold + ELU backward fused), weight + bias gradient (chunk partials + ordered sum), next to the forward launch and to ATen's
    convolution_backward on the same box (the vendor yardstick, NOT part of the product; it gets the already padded input and no ELU)."""
    import torch.nn.functional as F
    torch.manual_seed(0)
    B, T0 = 8, 720000
    PEAK = 157.3                                                  # TFLOP/s, v_mfma_f32_32x32x2_f32
    # (name, Cin, Cout, T, k, stride, dil, zero_pad, elu)
    shapes = [('enc first', 1, 32, T0, 7, 1, 1, False, False)]
    for c, t, s in ((32, T0, 2), (64, T0 // 2, 4), (128, T0 // 8, 5), (256, T0 // 40, 8)):
        shapes += [(f'unit{c} k7 d1', c, c, t, 7, 1, 1, False, True), (f'unit{c} k7 d9', c, c, t, 7, 1, 9, False, True),
                   (f'unit{c} k1', c, c, t, 1, 1, 1, False, True), (f'enc down s{s}', c, 2 * c, t, 2 * s, s, 1, False, False),
                   (f'dec up s{s} (k2 form)', 2 * c, s * c, t // s, 2, 1, 1, True, False)]
    shapes += [('enc last', 512, 512, T0 // 320, 3, 1, 1, False, False), ('dec first', 512, 512, T0 // 320, 7, 1, 1, False, False),
               ('dec last', 32, 1, T0, 7, 1, 1, False, False)]
    only = os.environ.get('KBENCH_CONVS_BWD_ATEN', '1') != '0'
    print(f'{"shape":48s} {"fwd":>8s} {"dgrad":>8s} {"TF":>6s} {"peak":>5s} {"wgrad":>8s} {"TF":>6s} {"peak":>5s} {"aten bwd":>9s} {"ours/aten":>9s}', flush=True)
    tot = [0.0, 0.0, 0.0, 0.0]
    for name, cin, cout, t, k, s, d, zp, elu in shapes:
        x = torch.randn(B, cin, t, device=dev) * 0.5
        w = torch.randn(cout, cin, k, device=dev) * (cin * k) ** -0.5
        b = torch.randn(cout, device=dev) * 0.1
        wp, wt = ops.conv1d_pack(w), ops.conv1d_pack_t(w)
        fwd = lambda: ops.conv1d_causal(x, wp, b, cout, k, stride=s, dilation=d, elu=elu, zero_pad=zp)      # noqa: E731
        y = fwd()
        g = torch.randn_like(y)
        ys = y if elu else None
        t_f = timeit(fwd, iters=3, warm=1)
        t_d = timeit(lambda: ops.conv1d_dgrad(g, ys, wt, cin, t, k, stride=s, dilation=d, zero_pad=zp), iters=3, warm=1)
        t_w = timeit(lambda: ops.conv1d_wgrad(g, ys, x, k, stride=s, dilation=d, zero_pad=zp), iters=3, warm=1)
        fl = 2.0 * y.numel() * cin * k / 1e9                      # GFLOP of each of fwd / dgrad / wgrad
        t_a = float('nan')
        if only:
            pad = d * (k - 1) + 1 - s
            xp = F.pad(x, (pad, 0)) if (zp or pad == 0) else F.pad(x, (pad, 0), mode='reflect')
            aten = lambda: torch.ops.aten.convolution_backward(g, xp, w, [cout], [s], [0], [d], False, [0], 1, [True, True, True])      # noqa: E731
            t_a = timeit(aten, iters=3, warm=1)
            del xp
        for i, v in enumerate((t_f, t_d, t_w, t_a)):
            tot[i] += v
        print(f'{name + f" {cin}->{cout} k{k} s{s} d{d} T={t}":48s} {t_f:8.3f} {t_d:8.3f} {fl / t_d:6.1f} {fl / t_d / PEAK:5.2f} {t_w:8.3f} {fl / t_w:6.1f} '
              f'{fl / t_w / PEAK:5.2f} {t_a:9.3f} {(t_d + t_w) / t_a:9.2f}', flush=True)
        del x, y, g, ys
    print(f'sum over the listed launches (ms): fwd {tot[0]:.2f}  dgrad {tot[1]:.2f}  wgrad {tot[2]:.2f}  aten bwd {tot[3]:.2f}')


def bench_local_attn_bwd():
    """LocalTransformer backward (csrc/local_attn_bwd.hip) at the default geometry, B = 8, dim 512, 8 heads x 64, window 128, T = 2250 frames (30 s at
    24 kHz / 320): the attention backward (dQ pass + dK/dV pass + scale finish, one call), LayerNorm backward and GEGLU backward next to their forward
    launches, the whole block forward and forward + backward, and decode(encode(x)) forward + backward with use_local_attn=True against False."""
    import torch.nn.functional as F
    from audiolm_pytorch_amd import soundstream as S
    torch.manual_seed(0)
    B, T, dim, H, dh, W = 8, 2250, 512, 8, 64, 128
    I = int(dim * 4 * 2 / 3)
    qkv, gates, do = torch.randn(B, 3 * H * dh, T, device=dev), torch.randn(B, H, T, device=dev), torch.randn(B, H * dh, T, device=dev)
    qs, ks = torch.ones(dh, device=dev), torch.ones(dh, device=dev)
    tabs = S._SinusoidalEmbeddings(dh, scale_base=W // 2).tables(2 * W, dev)
    fwd = lambda: ops.local_attn(qkv, qs, ks, *tabs, gates, H, dh, W, 8)      # noqa: E731
    o = fwd()
    t_f = timeit(fwd, iters=20, warm=3)
    t_b = timeit(lambda: ops.local_attn_bwd(qkv, qs, ks, *tabs, gates, o, do, H, dh, W, 8), iters=20, warm=3)
    nw = -(-T // W)
    # GFLOP of one dh-long pass over the visible (query, key) pairs; the forward makes 2 (q . k, p v), the backward 8 (dQ: q . k twice, dO . v, dS k;
    # dK/dV: q . k, dO . v, p dO, dS q)
    fl = 2.0 * B * H * dh * sum(min(i, W) + 1 for i in range(T)) / 1e9
    print(f'local_attn     fwd {t_f:7.3f} ms ({2 * fl / t_f:5.1f} TF fp32 VALU)   bwd (3 launches, {B * H * nw} workgroups x {W}) {t_b:7.3f} ms ({8 * fl / t_b:5.1f} TF)')
    x, dy = torch.randn(B, dim, T, device=dev), torch.randn(B, dim, T, device=dev)
    gamma, beta = torch.ones(dim, device=dev), torch.zeros(dim, device=dev)
    t_f = timeit(lambda: ops.layernorm_bct(x, gamma, beta), iters=20, warm=3)
    t_b = timeit(lambda: ops.layernorm_bct_bwd(dy, x, gamma, residual=dy), iters=20, warm=3)
    gb = x.numel() * 4 / 1e6
    print(f'layernorm_bct  fwd {t_f:7.3f} ms ({2 * gb / t_f:5.0f} GB/s)   bwd (dx + residual, dgamma / dbeta) {t_b:7.3f} ms ({5 * gb / t_b:5.0f} GB/s min. traffic)')
    u, dhh = torch.randn(B, 2 * I, T, device=dev), torch.randn(B, I, T, device=dev)
    t_f = timeit(lambda: ops.geglu_bct(u), iters=20, warm=3)
    t_b = timeit(lambda: ops.geglu_bct_bwd(dhh, u), iters=20, warm=3)
    gb = dhh.numel() * 4 / 1e6
    print(f'geglu_bct      fwd {t_f:7.3f} ms ({3 * gb / t_f:5.0f} GB/s)   bwd {t_b:7.3f} ms ({5 * gb / t_b:5.0f} GB/s)')
    lt = S.LocalTransformer(dim=dim, depth=1, heads=H, window_size=W, dim_head=dh).to(dev)
    xb = torch.randn(B, dim, T, device=dev)
    lt.eval()
    t_f = timeit(lambda: lt.run_bct(xb), iters=10, warm=2)
    lt.train()

    def step():
        lt.zero_grad(set_to_none=True)
        xg = xb.detach().requires_grad_()
        lt.run_bct(xg).backward(dy)
    t_fb = timeit(step, iters=10, warm=2)
    print(f'LocalTransformer block (depth 1) [B={B}, {dim}, T={T}]: forward {t_f:.3f} ms, forward + backward {t_fb:.3f} ms')
    wave = torch.randn(B, 1, T * 320, device=dev) * 0.1
    for local in (False, True):
        ss = A.SoundStream(codebook_size=4096, rq_num_quantizers=8, target_sample_hz=24000, strides=(2, 4, 5, 8), use_local_attn=local).to(dev).train()

        def cstep():
            ss.zero_grad(set_to_none=True)
            F.mse_loss(ss.decode(ss.encode(wave)), wave).backward()
        t = timeit(cstep, iters=3, warm=1)
        print(f'decode(encode(x)) forward + backward, 8 x 30 s @ 24 kHz, use_local_attn={local}: {t:.1f} ms')
        del ss


def bench_e2e():
    """BASELINE configs[4]: SoundStream(codebook 4096, 8 quantizers, 24 kHz) tokenize + CoarseTransformer(codebook 4096) step on 8 x 30 s of
    synthetic audio per GPU: N = 1 + 1501 + 1 + 6750 = 8253 tokens per sequence."""
    torch.manual_seed(0)
    ss = A.SoundStream(codebook_size=4096, rq_num_quantizers=8, target_sample_hz=24000, strides=(2, 4, 5, 8), use_local_attn=False)
    for r in ss.rq.rvqs:
        for q, l in enumerate(r.layers):
            l._codebook.embed.copy_(torch.randn(1, 4096, 512) * (0.5 ** q))
            l._codebook.initted.fill_(True)
    ss.to(dev)
    model = A.CoarseTransformer(dim=1024, depth=6, num_semantic_tokens=500, codebook_size=4096, num_coarse_quantizers=3, flash_attn=True).to(dev)
    w = A.CoarseTransformerWrapper(transformer=model, codec=ss, unique_consecutive=False, mask_prob=0.15)
    w.train()
    wave = torch.randn(8, 720000, device=dev) * 0.1
    sem = torch.randint(0, 500, (8, 1500), device=dev)

    def step():
        for p in model.parameters():
            p.grad = None
        loss = w(semantic_token_ids=sem, raw_wave=wave, return_loss=True)
        loss.backward()
        return loss
    t_tok = timeit(lambda: ss.tokenize(wave), iters=3, warm=1)
    t_all = timeit(step, iters=3, warm=1)
    ntok = 8 * 8253
    print(f'config-5 end to end (B=8, 30 s @ 24 kHz, N=8253): tokenize {t_tok:.1f} ms + transformer fwd+bwd {t_all - t_tok:.1f} ms = {t_all:.1f} ms/step '
          f'-> {ntok / t_all * 1e3:.0f} audio-tokens/s/GPU end to end, {ntok / (t_all - t_tok) * 1e3:.0f} transformer only')


def bench_models():
    """the other BASELINE configs on one GPU: configs[1] CoarseTransformer seq=1024, configs[2] FineTransformer seq=2049 (B=8, fwd+bwd)."""
    class Codec:
        rq_groups = 1
        num_quantizers = 8
    torch.manual_seed(0)
    cm = A.CoarseTransformer(dim=1024, depth=6, num_semantic_tokens=500, codebook_size=1024, num_coarse_quantizers=3, flash_attn=True).to(dev)
    cw = A.CoarseTransformerWrapper(transformer=cm, codec=Codec(), unique_consecutive=False, mask_prob=0.15)
    cw.train()
    sem, coarse = torch.randint(0, 500, (8, 253), device=dev), torch.randint(0, 1024, (8, 256, 3), device=dev)

    def cstep():
        for p in cm.parameters():
            p.grad = None
        cw(semantic_token_ids=sem, coarse_token_ids=coarse, return_loss=True).backward()
    t = timeit(cstep, iters=10, warm=3)
    print(f'configs[1] CoarseTransformer d=1024 depth=6 N=1024 B=8: {t:.2f} ms/step -> {8 * 1024 / t * 1e3:.0f} audio-tokens/s')
    del cm, cw
    fm = A.FineTransformer(dim=1024, depth=6, num_coarse_quantizers=3, num_fine_quantizers=5, codebook_size=1024, flash_attn=True).to(dev)
    fw = A.FineTransformerWrapper(transformer=fm, codec=Codec(), mask_prob=0.15)
    fw.train()
    grid = torch.randint(0, 1024, (8, 256, 8), device=dev)

    def fstep():
        for p in fm.parameters():
            p.grad = None
        fw(coarse_token_ids=grid[..., :3], fine_token_ids=grid[..., 3:], return_loss=True).backward()
    t = timeit(fstep, iters=10, warm=3)
    print(f'configs[2] FineTransformer d=1024 depth=6 N=2049 B=8: {t:.2f} ms/step -> {8 * 2049 / t * 1e3:.0f} audio-tokens/s')


def bench_bias():
    """`flash_attn=False` models: biased attention kernels vs the plain ones, the table MLP, and default-constructor model steps."""
    from audiolm_pytorch_amd import relpos
    B, N, H, dh = 8, 2048, 8, 64
    M = B * N
    Q, KV = rnd(M, H * dh), rnd(M, 2 * dh)
    K_, V_ = KV[:, :dh], KV[:, dh:]
    mask = (torch.rand(B, N, device=dev) > 0.15).to(torch.uint8)
    mask[:, 0] = 1
    dAO = rnd(M, H * dh)
    AO, LSE = ops.mqa_attn_fwd(Q, K_, V_, mask, B, N, H, dh)
    t0f = timeit(lambda: ops.mqa_attn_fwd(Q, K_, V_, mask, B, N, H, dh))
    t0b = timeit(lambda: ops.mqa_attn_bwd(Q, K_, V_, mask, AO, LSE, dAO, B, N, H, dh))
    print(f'plain attention  fwd {t0f:.3f} ms  bwd {t0b:.3f} ms')
    grid, findex = relpos.fine_index(765, 1281, 3, 5, dev)
    for name, index, LT in (('toeplitz', relpos.toeplitz_index(N, dev), 2 * N), ('coarse', relpos.toeplitz_index(N, dev, num_leading=1024), 2 * N),
                            ('fine', findex, grid.shape[0] + 1)):
        tbl = torch.randn(H, LT, device=dev)
        bias = relpos.AttnBias(tbl, *index)
        AOb, LSEb = ops.mqa_attn_fwd(Q, K_, V_, mask, B, N, H, dh, bias=bias)
        tf = timeit(lambda: ops.mqa_attn_fwd(Q, K_, V_, mask, B, N, H, dh, bias=bias))
        part = ops.attn_bias_part(B, N, H, LT, dev)
        tb = timeit(lambda: ops.mqa_attn_bwd(Q, K_, V_, mask, AOb, LSEb, dAO, B, N, H, dh, bias=bias, dtbl_part=part))
        tr = timeit(lambda: ops.attn_bias_grad_reduce(part, B, N, H))
        print(f'biased attention [{name}, LT={LT}]  fwd {tf:.3f} ms ({tf / t0f:.2f}x)  bwd {tb:.3f} ms ({tb / t0b:.2f}x)  table-grad reduce {tr:.3f} ms '
              f'(partials {part.numel() * 4 / 2**20:.0f} MiB)')
    rp = A.audiolm_pytorch.RelativePositionBias(dim=512, heads=8).to(dev)

    def table():
        for p in rp.parameters():
            p.grad = None
        b = rp(N, N)
        b.tbl.backward(torch.ones_like(b.tbl))
    t = timeit(table, iters=10, warm=3)
    print(f'RelativePositionBias table MLP (4095 rows, d=512) fwd+bwd: {t:.3f} ms')
    torch.manual_seed(0)
    for flash in (True, False):
        m = A.SemanticTransformer(dim=1024, depth=6, num_semantic_tokens=500, flash_attn=flash).to(dev)
        w = A.SemanticTransformerWrapper(transformer=m, unique_consecutive=False, mask_prob=0.15)
        w.train()
        ids = torch.randint(0, 500, (8, 2047), device=dev)

        def step():
            for p in m.parameters():
                p.grad = None
            w(semantic_token_ids=ids, return_loss=True).backward()
        t = timeit(step, iters=10, warm=3)
        print(f'SemanticTransformer d=1024 depth=6 N=2048 B=8 flash_attn={flash}: {t:.2f} ms/step -> {8 * 2048 / t * 1e3:.0f} tokens/s')
        del m, w


def bench_host():
    """is the headline step host-bound?  Python/ctypes time to ISSUE one step (no synchronisation) vs the GPU time of the step."""
    class Codec:
        rq_groups = 1
        num_quantizers = 8
    torch.manual_seed(0)
    m = A.CoarseTransformer(dim=1024, depth=6, num_semantic_tokens=500, codebook_size=1024, num_coarse_quantizers=3, flash_attn=True).to(dev)
    w = A.CoarseTransformerWrapper(transformer=m, codec=Codec(), unique_consecutive=False, mask_prob=0.15)
    w.train()
    sem, coarse = torch.randint(0, 500, (8, 509), device=dev), torch.randint(0, 1024, (8, 512, 3), device=dev)

    def step():
        m.transformer._cache.store.clear()
        for p in m.parameters():
            p.grad = None
        w(semantic_token_ids=sem, coarse_token_ids=coarse, return_loss=True).backward()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    n = 10
    issue = []
    t0 = time.perf_counter()
    for _ in range(n):
        a = time.perf_counter()
        step()
        issue.append(time.perf_counter() - a)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f'headline step: host issue time {sum(issue) / n * 1e3:.2f} ms/step (min {min(issue) * 1e3:.2f}), wall {(t2 - t0) / n * 1e3:.2f} ms/step, '
          f'GPU tail after the last issue {(t2 - t1) * 1e3:.2f} ms')
    import cProfile
    import pstats
    pr = cProfile.Profile()
    pr.enable()
    for _ in range(3):
        step()
    pr.disable()
    torch.cuda.synchronize()
    st = pstats.Stats(pr)
    st.sort_stats('tottime')
    st.print_stats(14)


def bench_gen():
    """autoregressive sampling throughput: SemanticTransformerWrapper.generate (d=1024, depth=6, B=8) with and without the kv cache"""
    torch.manual_seed(0)
    for flash in (True, False):
        m = A.SemanticTransformer(dim=1024, depth=6, num_semantic_tokens=500, flash_attn=flash).to(dev)
        w = A.SemanticTransformerWrapper(transformer=m, unique_consecutive=False)
        for use_cache, L in ((True, 512), (False, 128)):
            w.generate(max_length=8, batch_size=8, use_kv_cache=use_cache)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = w.generate(max_length=L, batch_size=8, use_kv_cache=use_cache)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f'generate semantic d=1024 depth=6 B=8 flash_attn={flash} kv_cache={use_cache}: {out.shape[1]} steps in {dt:.2f} s -> '
                  f'{dt / out.shape[1] * 1e3:.2f} ms/step, {8 * out.shape[1] / dt:.0f} tokens/s')
        del m, w


def bench_gen_notebook():
    """the three sampling rates the reference's demo notebook prints (audiolm_pytorch_demo.ipynb:603-605: Tesla T4, v0.7.5, no kv cache;
    semantic dim=1024, coarse / fine dim=512, depth 6, batch 1), on this path with the kv cache"""
    class Codec:
        rq_groups = 1
        num_quantizers = 8
    torch.manual_seed(0)
    sem = A.SemanticTransformer(dim=1024, depth=6, num_semantic_tokens=500).to(dev)
    sw = A.SemanticTransformerWrapper(transformer=sem, unique_consecutive=False)
    sw.generate(max_length=8, batch_size=1)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ids = sw.generate(max_length=256, batch_size=1)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f'semantic sampling (d=1024, depth 6, B=1, default ctor): {ids.shape[1] / dt:.1f} it/s   [notebook: 78.55 it/s on a T4, no kv cache]')
    coarse = A.CoarseTransformer(dim=512, depth=6, num_semantic_tokens=500, codebook_size=1024, num_coarse_quantizers=3).to(dev)
    cw = A.CoarseTransformerWrapper(transformer=coarse, codec=Codec(), unique_consecutive=False)
    s_ids = torch.randint(0, 500, (1, 256), device=dev)
    cw.generate(semantic_token_ids=s_ids, max_time_steps=2)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    c = cw.generate(semantic_token_ids=s_ids, max_time_steps=128)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f'coarse sampling (d=512, depth 6, 3 quantizers, B=1): {128 / dt:.1f} it/s (1 it = 3 tokens)   [notebook: 34.83 it/s]')
    fine = A.FineTransformer(dim=512, depth=6, num_coarse_quantizers=3, num_fine_quantizers=5, codebook_size=1024).to(dev)
    fw = A.FineTransformerWrapper(transformer=fine, codec=Codec())
    c_ids = torch.randint(0, 1024, (1, 128, 3), device=dev)
    fw.generate(coarse_token_ids=c_ids[:, :8])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    f = fw.generate(coarse_token_ids=c_ids)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f'fine sampling (d=512, depth 6, 3 + 5 quantizers, B=1): {128 / dt:.1f} it/s (1 it = 5 tokens)   [notebook: 2.91 it/s]')


def bench_misc():
    M, D, I, Ip = 16384, 1024, 2730, 2736
    U = rnd(M, 2 * Ip)
    g3 = torch.ones(I, device=dev)
    HN, mean3, rstd3 = ops.geglu_ln_fwd(U, g3, I, Ip)
    t = timeit(lambda: ops.geglu_ln_fwd(U, g3, I, Ip))
    print(f'geglu_ln_fwd: {t:.3f} ms  {(M * 3 * Ip * 2) / t / 1e6:.0f} GB/s')
    dHN = rnd(M, Ip)
    t = timeit(lambda: ops.geglu_ln_bwd(dHN, U, g3, mean3, rstd3, I, Ip))
    print(f'geglu_ln_bwd: {t:.3f} ms  {(M * 5 * Ip * 2) / t / 1e6:.0f} GB/s')
    x = rnd(M, D)
    g = torch.ones(D, device=dev)
    y, _, mean, rstd = ops.layernorm_fwd(x, g)
    t = timeit(lambda: ops.layernorm_fwd(x, g))
    print(f'layernorm_fwd bf16: {t:.3f} ms  {(M * D * 4) / t / 1e6:.0f} GB/s')
    dy = rnd(M, D)
    t = timeit(lambda: ops.layernorm_bwd(dy, x, mean, rstd, g))
    print(f'layernorm_bwd: {t:.3f} ms  {(M * D * 8) / t / 1e6:.0f} GB/s')


def bench_t5():
    """native T5Encoder.forward at t5-v1_1-base size against the plain-torch restatement (tests/t5_restated.py) in fp32 eager torch on the same GPU in
    the same process: what a user of text= has without this package's encoder.  One event pair per forward, median of 30 after 5 warm-up runs."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import t5_restated as TR
    sd = TR.random_state_dict(11)
    enc = A.T5Encoder.from_state_dict(sd, num_heads=12).to(dev)
    sdg = {k: v.to(dev) for k, v in sd.items()}
    mmac = lambda T: 12 * (4 * 768 * 768 + 3 * 768 * 2048 + 2 * T * 768) / 1e6                   # noqa: E731  per token

    def median_ms(fn, iters=30, warm=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]
    for B, T, lengths in ((8, 256, [256, 1, 17, 100, 255, 33, 64, 200]), (8, 24, [24, 10, 17, 12, 21, 5, 14, 19])):
        ids = torch.randint(0, 512, (B, T), device=dev)
        mask = (torch.arange(T, device=dev)[None, :] < torch.tensor(lengths, device=dev)[:, None]).long()
        pb = TR.position_bias(sd[TR.BIAS_KEY], T).to(dev)          # once, outside the timed call: transformers builds its bias on the device
        with torch.no_grad():
            nat = median_ms(lambda: enc(ids, mask))
            ref = median_ms(lambda: TR.encode(sdg, ids, mask, heads=12, gated=True, bias=pb))
            err = relerr(enc(ids, mask), TR.encode(sdg, ids, mask, heads=12, gated=True))
        flop = 2 * mmac(T) * 1e6 * B * T
        floor = flop / 157.3e12 * 1e3
        print(f't5 v1.1-base {B} x {T}: native {nat[0]:.3f} ms (min {nat[1]:.3f}, max {nat[2]:.3f}; {flop / nat[0] / 1e9:.1f} TFLOP/s, '
              f'{nat[0] / floor:.2f} x the {floor:.3f} ms fp32 matrix-peak floor)   eager torch fp32 {ref[0]:.3f} ms (min {ref[1]:.3f}, max {ref[2]:.3f})   '
              f'native / eager {nat[0] / ref[0]:.2f}   max rel diff {err:.1e}')


def bench_rvq_train():
    """train-mode residual VQ at the workload shape (8 x 30 s @ 24 kHz: M = 18 000 frames, d = 512, C = 1024, Q = 8, one group): the training forward
    (all layers active, no init step), the per-code statistics kernel alone (uniform codes, and 90 % of the rows on four codes), the backward, the eval
    alm_rvq_encode of the same shape, and as a yardstick the dense formulation the reference runs for the statistics -- einsum('nd,nc->cd') with the
    one-hot matrix plus its column sum -- in ATen fp32 on the same GPU.  Median of 20 after 3 warm-up runs, one event pair per call."""
    from audiolm_pytorch_amd import soundstream as S
    M, d, C, Q = 18000, 512, 1024, 8

    def median_ms(fn, iters=20, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2]
    torch.manual_seed(0)
    rq = S.GroupedResidualVQ(dim=d, num_quantizers=Q, codebook_size=C, quantize_dropout=False)
    for q, l in enumerate(rq.rvqs[0].layers):
        cb = l._codebook
        cb.embed.copy_(torch.randn(1, C, d) * 0.7 ** q), cb.cluster_size.fill_(M / C), cb.embed_avg.copy_(cb.embed * (M / C)), cb.initted.fill_(True)
    rq = rq.to(dev)
    x = torch.randn(1, M, d, device=dev)
    rq.eval()
    with torch.no_grad():
        t_eval = median_ms(lambda: rq(x))
    rq.train()
    with torch.no_grad():
        t_fwd = median_ms(lambda: rq(x))
    xg = x.clone().requires_grad_()
    out, _, losses = rq(xg)
    g = torch.randn_like(out)
    t_bwd = median_ms(lambda: torch.autograd.grad([out, losses], [xg], [g, torch.ones_like(losses)], retain_graph=True))
    r = x[0]
    for name, idx in (('uniform codes', torch.randint(0, C, (M,), device=dev)),
                      ('90 % of the rows on 4 codes', torch.where(torch.rand(M, device=dev) < 0.9, torch.randint(0, 4, (M,), device=dev), torch.randint(0, C, (M,), device=dev)))):
        t_stats = median_ms(lambda: ops.rvq_code_stats(r, idx, C))

        def dense():
            onehot = torch.nn.functional.one_hot(idx, C).to(F32)
            return torch.einsum('nd,nc->cd', r, onehot), onehot.sum(0)
        t_dense = median_ms(dense)
        n, s = ops.rvq_code_stats(r, idx, C)
        rs, rn = dense()
        print(f'rvq_train stats {M} x {d} -> {C} codes, {name}: {t_stats:.3f} ms ({(M * d + C * d) * 4 / t_stats / 1e6:.0f} GB/s of rows + sums)   '
              f'dense one-hot einsum + sum in ATen fp32 {t_dense:.3f} ms ({2 * C * M * d / t_dense / 1e9:.1f} TFLOP/s)   ratio {t_dense / t_stats:.1f}   '
              f'counts equal {bool(torch.equal(n, rn))}  max rel diff of the sums {relerr(s, rs):.1e}')
    print(f'rvq_train forward {M} frames x {Q} x {C} codes, d {d}: {t_fwd:.2f} ms   eval alm_rvq_encode {t_eval:.2f} ms   forward / eval {t_fwd / t_eval:.2f}   '
          f'backward {t_bwd:.2f} ms')


def bench_discr():
    """wave discriminators of SoundStream training at 8 x 1 s and 8 x 10 s of 16 kHz audio (real and fake as one batch of 16): forward + backward of one
    MultiScaleDiscriminator (input and parameter gradients), each of its seven layers alone, and the whole discriminator-loss step (three scales, the
    pooling between them, hinge means, backward into all 16.9 M parameters) on the kernels of csrc/discr.hip, against the SAME modules run by PyTorch-ROCm
    (F.conv1d / F.leaky_relu / F.avg_pool1d / F.relu, fp32) on the same box.  Interleaved: each round times the hand path, then ATen; medians of the
    rounds, one event pair per call."""
    import torch.nn.functional as F
    from audiolm_pytorch_amd import discriminators as D

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def pair(ours, aten, rounds=10, warm=2):
        for _ in range(warm):
            ours(), aten()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(rounds):
            a.append(once(ours)), b.append(once(aten))
        a.sort(), b.sort()
        return a[len(a) // 2], b[len(b) // 2]

    def aten_discr(m, x):
        x = m.init_conv(x)
        inter = []
        for layer in m.conv_layers:
            x = F.leaky_relu(layer[0](x), 0.1)
            inter.append(x)
        return m.final_conv[2](F.leaky_relu(m.final_conv[0](x), 0.1)), inter

    def fwd_bwd(run, m, x):
        logits, inter = run(m, x)
        loss = logits.mean() + sum(t.mean() for t in inter)
        torch.autograd.grad(loss, [x, *m.parameters()])

    torch.manual_seed(0)
    discrs = [A.MultiScaleDiscriminator().to(dev) for _ in range(3)]
    downs = [None, D.AvgPoolDownsample(2), D.AvgPoolDownsample(2)]
    m = discrs[0]
    for secs in (1, 10):
        T = 16000 * secs
        real, fake = torch.randn(8, 1, T, device=dev) * 0.3, torch.randn(8, 1, T, device=dev) * 0.3
        x = torch.cat((real, fake)).requires_grad_()
        t_o, t_a = pair(lambda: fwd_bwd(lambda mm, xx: mm(xx, return_intermediates=True), m, x), lambda: fwd_bwd(aten_discr, m, x))
        print(f'discr 8 x {secs} s: one MultiScaleDiscriminator fwd + bwd (batch 16 x {T}): hand {t_o:.2f} ms   ATen {t_a:.2f} ms   hand / ATen {t_o / t_a:.2f}', flush=True)
        h = x.detach()
        convs = [('init_conv', m.init_conv, False), *((f'conv_layers.{i}', l[0], True) for i, l in enumerate(m.conv_layers)),
                 ('final_conv.0', m.final_conv[0], True), ('final_conv.2', m.final_conv[2], False)]
        for name, conv, leaky in convs:
            hin = h.clone().requires_grad_()

            def ours_layer():
                y = D.conv1d_act(conv, hin, leaky=leaky)
                torch.autograd.grad(y.mean(), [hin, conv.weight, conv.bias])

            def aten_layer():
                y = conv(hin)
                y = F.leaky_relu(y, 0.1) if leaky else y
                torch.autograd.grad(y.mean(), [hin, conv.weight, conv.bias])
            t_o, t_a = pair(ours_layer, aten_layer, rounds=6)
            print(f'    {name:14s} {conv.in_channels:5d} -> {conv.out_channels:5d} k{conv.kernel_size[0]} s{conv.stride[0]} g{conv.groups:<4d} T_in {hin.shape[-1]:7d}: '
                  f'hand {t_o:.3f} ms   ATen {t_a:.3f} ms   hand / ATen {t_o / t_a:.2f}', flush=True)
            with torch.no_grad():
                h = D.conv1d_act(conv, hin.detach(), leaky=leaky)
        params = [p for d in discrs for p in d.parameters()]

        def ours_step():
            scaled, losses = torch.cat((real, fake)), []
            for d, down in zip(discrs, downs):
                scaled = scaled if down is None else down(scaled)
                logits = d(scaled)
                losses.append(D.hinge_discr_loss(logits[8:], logits[:8]))
            torch.autograd.grad(torch.stack(losses).mean(), params)

        def aten_step():
            r, f, losses = real, fake, []
            for d, down in zip(discrs, downs):
                if down is not None:
                    r, f = F.avg_pool1d(r, 4, stride=2, padding=2), F.avg_pool1d(f, 4, stride=2, padding=2)
                rl, fl = aten_discr(d, r)[0], aten_discr(d, f)[0]
                losses.append((F.relu(1 + fl) + F.relu(1 - rl)).mean())
            torch.autograd.grad(torch.stack(losses).mean(), params)
        t_o, t_a = pair(ours_step, aten_step)
        print(f'discr 8 x {secs} s: discriminator-loss step (3 scales, fwd + bwd): hand {t_o:.2f} ms   ATen {t_a:.2f} ms   hand / ATen {t_o / t_a:.2f}', flush=True)


def bench_stft_discr():
    """ComplexSTFTDiscriminator of SoundStream training at 8 x 1 s and 8 x 10 s of 16 kHz audio (real and fake as one batch of 16): forward + backward
    of the native module at its defaults (input and parameter gradients) and each of its conv forms alone (forward + dgrad + wgrad) on the kernels of
    csrc/stft_discr.hip, against the SAME computation issued through PyTorch-ROCm (tests/stft_discr_restated.py moved to the GPU: torch.stft + complex
    F.conv2d, fp32) on the same box.  The conv launches' achieved FLOP/s (8 real FLOP per complex multiply-accumulate) is printed as a fraction of
    the 155 TFLOP/s exact-fp32 matrix peak.  Interleaved rounds, medians, one event pair per call."""
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    from stft_discr_restated import ComplexSTFTDiscriminatorRestated
    from audiolm_pytorch_amd import ops
    PEAK = 155e12

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds, warm):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [sorted(t)[len(t) // 2] for t in ts]

    torch.manual_seed(0)
    m = A.ComplexSTFTDiscriminator().to(dev)
    ref = ComplexSTFTDiscriminatorRestated()
    ref.load_state_dict(m.state_dict())
    ref.to(dev)
    aten_ok = True
    try:
        ref(torch.randn(1, 1, 4096, device=dev))[0].sum().backward()
        torch.cuda.synchronize()
    except Exception as e:                                       # no complex conv on this build: say so and time ours alone
        aten_ok = False
        print(f'stft_discr: ATen cannot run the complex conv on this build ({type(e).__name__}: {str(e)[:120]}); timing the native path alone', flush=True)

    def fwd_bwd(mod, x):
        logits, inter = mod(x, return_intermediates=True)
        loss = logits.mean() + sum(torch.view_as_real(t).mean() for t in inter)
        torch.autograd.grad(loss, [x, *mod.parameters()])

    for secs in (1, 10):
        n = 16000 * secs
        x = (torch.randn(16, 1, n, device=dev) * 0.3).requires_grad_()
        rounds, warm = (8, 2) if secs == 1 else (3, 1)
        fns = [lambda: fwd_bwd(m, x)] + ([lambda: fwd_bwd(ref, x)] if aten_ok else [])
        ts = median(fns, rounds, warm)
        tail = f'   ATen {ts[1]:.2f} ms   hand / ATen {ts[0] / ts[1]:.2f}' if aten_ok else ''
        print(f'stft_discr 8 x {secs} s: ComplexSTFTDiscriminator fwd + bwd (batch 16 x {n}): hand {ts[0]:.2f} ms{tail}', flush=True)
        basis = ops.stft_basis(m.n_fft, torch.hann_window(m.win_length), False, dev)
        with torch.no_grad():
            h = ops.stft(x.detach().reshape(16, n), basis, m.n_fft, m.hop_length).unsqueeze(1)
        for name, conv in [('init_conv', m.init_conv), *((f'layers.{i}.{j}', c) for i, l in enumerate(m.layers)
                                                         for j, c in (('0.fn.0', l[0].fn[0]), ('1', l[1]))), ('final_conv', m.final_conv)]:
            hin = h.clone().requires_grad_()
            wc, bc = torch.view_as_complex(conv.weight.detach()).requires_grad_(), torch.view_as_complex(conv.bias.detach()).requires_grad_()
            hc = torch.view_as_complex(hin.detach()).requires_grad_()

            def ours_layer():
                y = conv(hin)
                torch.autograd.grad(y.mean(), [hin, conv.weight, conv.bias])

            def aten_layer():
                y = F.conv2d(hc, wc, bc, stride=conv.stride, padding=conv.padding)
                torch.autograd.grad(torch.view_as_real(y).mean(), [hc, wc, bc])
            ts = median([ours_layer] + ([aten_layer] if aten_ok else []), rounds, warm)
            with torch.no_grad():
                y = conv(hin.detach())
            Cout, Cin, kh, kw, _ = conv.weight.shape
            flop = 3 * 8. * Cout * Cin * kh * kw * y.shape[0] * y.shape[2] * y.shape[3]            # forward + dgrad + wgrad
            rate = flop / (ts[0] * 1e-3)
            tail = f'   ATen {ts[1]:.3f} ms   hand / ATen {ts[0] / ts[1]:.2f}' if aten_ok else ''
            print(f'    {name:16s} {Cin:4d} -> {Cout:4d} k{kh}x{kw} s{conv.stride} in {tuple(hin.shape[2:4])}: hand {ts[0]:.3f} ms '
                  f'({rate / 1e12:.2f} TFLOP/s, {100 * rate / PEAK:.1f} % of the fp32 matrix peak){tail}', flush=True)
            h = y
            if name.endswith('0.fn.0'):                          # the unit's second 3 x 3 conv has the first one's form: step over it
                with torch.no_grad():
                    h = hin.detach()


def bench_mel_loss():
    """Multi-spectral mel reconstruction loss of SoundStream training at 8 x 1 s and 8 x 3 s of 16 kHz audio: forward + backward (d / d recon) of the
    six-scale term at the reference defaults on the kernels of csrc/mel_loss.hip, against the SAME computation issued through PyTorch-ROCm
    (tests/mel_restated.py moved to the GPU: torch.stft + matmul + autograd, fp32) on the same box; then every scale alone, and the native launches of
    each scale one by one.  Interleaved rounds, medians, one event pair per call."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    from mel_restated import MelSpectrogramRestated, multi_spectral_recon_loss_restated

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds=10, warm=3):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [sorted(t)[len(t) // 2] for t in ts]

    ours, refs, alphas = [], [], []
    for p in range(6, 12):
        win = 2 ** p
        kw = dict(sample_rate=16000, n_fft=max(512, win), win_length=win, hop_length=win // 4, n_mels=64, normalized=False)
        ours.append(A.MelSpectrogram(**kw).to(dev))
        refs.append(MelSpectrogramRestated(**kw).float().to(dev))
        alphas.append((win / 2) ** 0.5)

    def hand(ts, al, orig, recon):
        torch.autograd.grad(A.multi_spectral_recon_loss(orig, recon, ts, al), [recon])

    def aten(ts, al, orig, recon):
        torch.autograd.grad(multi_spectral_recon_loss_restated(orig, recon, ts, al), [recon])

    for secs in (1, 3):
        n = 16000 * secs
        orig, recon = torch.randn(8, 1, n, device=dev) * 0.3, (torch.randn(8, 1, n, device=dev) * 0.3).requires_grad_()
        t_o, t_a = median([lambda: hand(ours, alphas, orig, recon), lambda: aten(refs, alphas, orig, recon)])
        print(f'mel_loss 8 x {secs} s: six-scale term fwd + bwd: hand {t_o:.3f} ms   ATen {t_a:.3f} ms   hand / ATen {t_o / t_a:.2f}   '
              '(per scale: 4 launches forward, 4 backward)', flush=True)
        both = torch.cat((orig, recon.detach())).reshape(16, n)
        g = torch.ones((), device=dev)
        for t, r, alpha in zip(ours, refs, alphas):
            t_o, t_a = median([lambda: hand([t], [alpha], orig, recon), lambda: aten([r], [alpha], orig, recon)])
            basis, fb, left = t._dft_basis(dev), t.mel_scale.fb, (t.n_fft - t.win_length) // 2
            P, X = ops.mel_power(both, basis, t.n_fft, t.hop_length, left, left + t.win_length, x_from=8)
            mel = ops.mel_project(P, fb)
            _, _, norms = ops.mel_frame_loss(mel, alpha)
            dmel = ops.mel_frame_loss_bwd(mel, norms, g, alpha)
            dX = ops.mel_power_bwd(dmel, fb, X)
            parts = median([lambda: ops.mel_power(both, basis, t.n_fft, t.hop_length, left, left + t.win_length, x_from=8), lambda: ops.mel_project(P, fb),
                            lambda: ops.mel_frame_loss(mel, alpha), lambda: ops.mel_frame_loss_bwd(mel, norms, g, alpha),
                            lambda: ops.mel_power_bwd(dmel, fb, X), lambda: ops.stft_bwd(dX, basis, n, t.n_fft, t.hop_length)])
            names = ('power', 'project', 'frame loss (2)', 'column grad', 'dP -> dX', 'stft bwd (2)')
            print(f'    win {t.win_length:4d} n_fft {t.n_fft:4d} hop {t.hop_length:3d} T {mel.shape[-1]:5d}: hand {t_o:.3f} ms   ATen {t_a:.3f} ms   hand / ATen '
                  f'{t_o / t_a:.2f}   launches: ' + ', '.join(f'{k} {v * 1e3:.0f} us' for k, v in zip(names, parts)), flush=True)


def bench_grad_penalty():
    """Discriminator step of SoundStream training with and without the gradient penalty at a training-like shape: B = 8, one second at 24 kHz, the
    three default MultiScaleDiscriminators and the default ComplexSTFTDiscriminator.  One step = the discriminator branch with
    return_discr_losses_separately=True on fixed real / fake waves (the codec is left out), then backward over every package entry with
    retain_graph=True, as the reference's trainer does.  Beside it, as a yardstick, the wave discriminators' penalties alone (three scales, real and
    fake, each entry's backward) on the native double backward and composed from torch's own conv1d + autograd (ATen, fp32) on the same box.
    Interleaved rounds, medians, one event pair per call."""
    import torch.nn.functional as F
    from audiolm_pytorch_amd import discriminators as D

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds=10, warm=3):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [sorted(t)[len(t) // 2] for t in ts]

    B, n = 8, 24000
    torch.manual_seed(0)
    ss = A.SoundStream(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False, multi_spectral_recon_loss_weight=0.,
                       stft_discriminator=True, with_discriminators=True, with_grad_penalty=True).to(dev).train()
    real, fake = torch.randn(B, 1, n, device=dev) * 0.3, torch.randn(B, 1, n, device=dev) * 0.3

    def step(penalty):
        ss.zero_grad(set_to_none=True)
        for _, loss in ss._discr_loss(real, fake, True, penalty):
            loss.backward(retain_graph=True)

    t_plain, t_pen = median([lambda: step(False), lambda: step(True)])
    print(f'grad_penalty {B} x {n}: discriminator step, backward per package entry: without the penalty (4 entries) {t_plain:.2f} ms   with it (8 entries) '
          f'{t_pen:.2f} ms   ratio {t_pen / t_plain:.2f}', flush=True)

    def aten_discr(m, x):
        x = m.init_conv(x)
        for layer in m.conv_layers:
            x = F.leaky_relu(layer[0](x), 0.1)
        return m.final_conv[2](F.leaky_relu(m.final_conv[0](x), 0.1))

    def aten_penalty(wave, loss):
        g, = torch.autograd.grad(loss, wave, torch.ones_like(loss), create_graph=True)
        return 10 * (torch.linalg.vector_norm(g.reshape(g.shape[0], -1), dim=1) ** 2).mean()

    def wave_penalties(native):
        ss.zero_grad(set_to_none=True)
        scaled = torch.cat((real, fake))
        for d, down in zip(ss.discriminators, ss.downsamples):
            scaled = down(scaled)
            if native:
                wave = scaled.detach().requires_grad_()
                logits = d(wave)
                pens = ss._penalty_pair(wave, D.hinge_discr_loss(logits[B:], logits[:B]), B)
            else:
                r, f = scaled[:B].detach().requires_grad_(), scaled[B:].detach().requires_grad_()
                loss = (F.relu(1 + aten_discr(d, f)) + F.relu(1 - aten_discr(d, r))).mean()
                pens = aten_penalty(r, loss), aten_penalty(f, loss)
            for p in pens:
                p.backward(retain_graph=True)

    try:
        t_o, t_a = median([lambda: wave_penalties(True), lambda: wave_penalties(False)])
        print(f'grad_penalty {B} x {n}: wave discriminators\' penalties alone (3 scales x real, fake; fwd + double backward per entry): hand {t_o:.2f} ms   '
              f'ATen {t_a:.2f} ms   hand / ATen {t_o / t_a:.2f}', flush=True)
    except Exception as e:                                       # the yardstick is optional: say so and keep the native numbers
        t_o, = median([lambda: wave_penalties(True)])
        print(f'grad_penalty {B} x {n}: wave discriminators\' penalties alone: hand {t_o:.2f} ms   ATen did not run ({type(e).__name__}: {e})', flush=True)


def bench_se_film():
    """Squeeze-excite of the ResidualUnit and the FiLM conditioners (csrc/film_se.hip) at the default codec's unit shapes (8 x 10 s @ 16 kHz:
    C = 32 / 64 / 128 / 256 at T = 160000 / 80000 / 20000 / 4000, hidden width max(8, C / 4)): the gate's forward and backward launches with the
    rate on the bytes the op must move (12 B per element: u, residual, out; g, u, du), and beside them, same box and same run, a whole unit without
    and with squeeze-excite: eval forward, and training forward + backward.  Interleaved rounds, medians, one event pair per call."""
    from audiolm_pytorch_amd import soundstream as S

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds=7, warm=2):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [sorted(t)[len(t) // 2] for t in ts]

    torch.manual_seed(0)
    B, n = 8, 160000
    print(f'{"shape":28s} {"se fwd":>8s} {"GB/s":>6s} {"se bwd":>8s} {"GB/s":>6s} | {"unit fwd":>9s} {"+SE":>8s} {"ratio":>6s} | {"unit f+b":>9s} {"+SE":>8s} {"ratio":>6s}',
          flush=True)
    for C, T in ((32, n), (64, n // 2), (128, n // 8), (256, n // 40)):
        inner = max(8, C // 4)
        u, res, g = (torch.randn(B, C, T, device=dev) for _ in range(3))
        w1, b1 = torch.randn(inner, C, 1, device=dev) * C ** -0.5, torch.randn(inner, device=dev) * 0.1
        w2, b2 = torch.randn(C, inner, 1, device=dev) * inner ** -0.5, torch.randn(C, device=dev) * 0.1
        t_f, t_b = median([lambda: ops.se_gate_fwd(u, w1, b1, w2, b2, residual=res), lambda: ops.se_gate_bwd(g, u, w1, b1, w2, b2)])
        gb = 12.0 * u.numel() / 1e6                               # MB per launch on the minimum traffic; / ms = GB/s
        plain, se = (S.ResidualUnit(C, C, 3, squeeze_excite=flag).to(dev) for flag in (False, True))
        ug = u.detach().requires_grad_()

        def fwd(unit):
            with torch.no_grad():
                return unit.eval()(u)

        def step(unit):
            unit.train().zero_grad(set_to_none=True)
            ug.grad = None
            unit(ug).backward(g)                                  # the input gradient too, as inside the stack

        f0, f1 = median([lambda: fwd(plain), lambda: fwd(se)])
        s0, s1 = median([lambda: step(plain), lambda: step(se)], rounds=5)
        print(f'{f"C={C} inner={inner} T={T}":28s} {t_f:8.3f} {gb / t_f:6.0f} {t_b:8.3f} {gb / t_b:6.0f} | {f0:9.3f} {f1:8.3f} {f1 / f0:6.2f} | '
              f'{s0:9.3f} {s1:8.3f} {s1 / s0:6.2f}', flush=True)
        del u, ug, res, g, plain, se
    rows, C = 8 * 500, 512                                        # the default codebook_dim at 8 x 10 s
    x, gy = torch.randn(rows, C, device=dev), torch.randn(rows, C, device=dev)
    w, b = torch.randn(2 * C, 2, device=dev), torch.randn(2 * C, device=dev)
    t_f, t_b = median([lambda: ops.film_fwd(x, w, b, 1., 0.), lambda: ops.film_bwd(gy, x, w, b, 1., 0.)])
    print(f'film [{rows} x {C}]: fwd {t_f * 1e3:.1f} us   bwd (2 launches) {t_b * 1e3:.1f} us', flush=True)


def bench_fsq():
    """Residual FSQ (csrc/fsq.hip) at 8 x 30 s of 16 kHz audio / 320 = 12 000 tokens, dim 512, levels [8, 5, 5, 5], Q = 8, all layers active:
    alm_fsq_fwd and alm_fsq_bwd (two launches) beside the same arithmetic written in ATen ops (forward: addmm, the Q-layer chain, addmm; backward:
    torch autograd of that forward with straight-through rounding), same process, interleaved rounds, medians, one event pair per call.  The rate is
    on the bytes the op must move (forward: x in, out out = 2 M dim 4 B; backward: g and x in, dx out = 3 M dim 4 B) and is set against the 8 TB/s
    HBM peak; at this size every operand also fits the 256 MB last-level cache, so the rate is not an HBM measurement."""
    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds=31, warm=5):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [(sorted(t)[len(t) // 2], sorted(t)[0], sorted(t)[-1]) for t in ts]

    torch.manual_seed(0)
    M, dim, levels, Q = 12000, 512, (8, 5, 5, 5), 8
    d, k = len(levels), Q - 1
    x, g = torch.randn(M, dim, device=dev), torch.randn(M, dim, device=dev)
    weights = (torch.randn(d, dim, device=dev) * (1.5 / dim ** 0.5), torch.randn(d, device=dev) * 0.1, torch.randn(dim, d, device=dev) * 0.5,
               torch.randn(dim, device=dev) * 0.1)
    table = ops.fsq_constants(levels, Q)
    consts = table.to(dev)
    head = table[:56].reshape(7, 8)[:, :d].to(dev)
    half_l, offset, shift, _, half_w, basis, _ = head
    scale = table[56:56 + 8 * Q].reshape(Q, 8)[:, :d].to(dev)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    idx = torch.empty(M, Q, dtype=torch.int64, device=dev)
    z = ops.fsq_fwd(x, weights, consts, d, Q, k, idx, out, save_z=True)

    def aten_fwd(x, w_in, b_in, w_out, b_out):
        r = torch.addmm(b_in, x, w_in.t())
        zsum, inds = 0., []
        for q in range(Q):
            b = torch.tanh(r / scale[q] + shift) * half_l - offset
            code = b + (torch.round(b) - b).detach()
            inds.append(((code.detach() + half_w) * basis).sum(-1).long())
            quant = code / half_w * scale[q]
            r, zsum = r - quant.detach(), zsum + quant
        return torch.addmm(b_out, zsum, w_out.t()), torch.stack(inds, dim=-1)

    leaves = [t.detach().clone().requires_grad_() for t in (x, *weights)]
    a_out, a_idx = aten_fwd(*leaves)

    def aten_fwd_nograd():
        with torch.no_grad():
            return aten_fwd(x, *weights)

    print(f'fsq [{M} x {dim}], levels {list(levels)}, Q {Q}: indices equal to the ATen chain on {float((a_idx == idx).all(dim=-1).float().mean()):.4%} of '
          f'the tokens, out rel-max {relerr(out, a_out.detach()):.2e}', flush=True)
    fns = [lambda: ops.fsq_fwd(x, weights, consts, d, Q, k, idx, out, save_z=True), aten_fwd_nograd,
           lambda: ops.fsq_bwd(g, x, z, weights, consts, d, Q, k, dx), lambda: torch.autograd.grad(a_out, leaves, g, retain_graph=True)]
    mb = M * dim * 4 / 1e6
    for (name, nbytes), (med, lo, hi) in zip((('alm_fsq_fwd', 2 * mb), ('ATen fwd (no grad)', 2 * mb), ('alm_fsq_bwd (2 launches)', 3 * mb),
                                              ('ATen autograd bwd', 3 * mb)), median(fns)):
        print(f'  {name:26s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})   {nbytes / med:7.0f} GB/s on the minimum traffic = '
              f'{nbytes / med / 8000:.1%} of the 8 TB/s HBM peak', flush=True)


def bench_lfq():
    """Residual LFQ (csrc/lfq.hip) at 8 x 45 s of 16 kHz audio / 320 = 18 000 tokens, dim 512, 1024 codes (d = 10), Q = 8, all layers active, training
    mode: alm_lfq_fwd (three launches: projection + chain, the code statistics, the finish) and alm_lfq_bwd (three launches, the loss gradient
    included) beside (a) the dense torch formulation of tests/lfq_restated.py in fp32 on the same GPU (explicit [1024, 10] codebook, einsum, softmax,
    clamped log, autograd) and (b) the FSQ kernels at the same M / dim ([8, 5, 5, 5], Q = 8).  Same process, interleaved rounds, medians, one event
    pair per call.  The LFQ work is arithmetic, not traffic: M Q 2^d = 147 M probabilities per pass, each formed in double."""
    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds=15, warm=3):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [(sorted(t)[len(t) // 2], sorted(t)[0], sorted(t)[-1]) for t in ts]

    torch.manual_seed(0)
    M, dim, d, Q = 8 * 2250, 512, 10, 8
    k, cfg = Q - 1, (ops.LFQ_INV_TEMPERATURE, 0.1, 0.25, 1.)
    tau, w_e, w_c, gamma = cfg
    x, g = torch.randn(M, dim, device=dev), torch.randn(M, dim, device=dev)
    g_loss = torch.randn(Q, device=dev)
    weights = (torch.randn(d, dim, device=dev) * (1.5 / dim ** 0.5), torch.randn(d, device=dev) * 0.1, torch.randn(dim, d, device=dev) * 0.5,
               torch.randn(dim, device=dev) * 0.1)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    idx = torch.empty(M, Q, dtype=torch.int64, device=dev)
    ws_f = torch.empty(_lib.query('alm_lfq_fwd_ws_doubles', M, d, Q), dtype=torch.float64, device=dev)
    ws_b = torch.empty(_lib.query('alm_lfq_bwd_ws_floats', M, dim, d, Q), device=dev)
    z, losses, avg = ops.lfq_fwd(x, weights, d, Q, k, idx, out, loss_cfg=cfg, ws=ws_f)
    mask = 2 ** torch.arange(d - 1, -1, -1, device=dev)
    sigma = ((torch.arange(2 ** d, device=dev)[:, None] & mask) != 0).float() * 2 - 1

    def dense_fwd(x, w_in, b_in, w_out, b_out):
        r = torch.addmm(b_in, x, w_in.t())
        zsum, inds, ls = 0., [], []
        for q in range(Q):
            s = 2. ** -q
            hard = torch.where(r > 0, s, -s).detach()
            inds.append(((r > 0).long() * mask).sum(-1))
            p = (2 * tau * torch.einsum('md,cd->mc', r, sigma * s)).softmax(dim=-1)
            avg_p = p.mean(dim=0)
            ent = (-p * torch.log(p.clamp(min=1e-5))).sum(-1).mean() - gamma * (-avg_p * torch.log(avg_p.clamp(min=1e-5))).sum()
            ls.append(w_e * ent + w_c * torch.nn.functional.mse_loss(r, hard))
            zsum, r = zsum + r + (hard - r).detach(), r - hard
        return torch.addmm(b_out, zsum, w_out.t()), torch.stack(inds, dim=-1), torch.stack(ls)

    leaves = [t.detach().clone().requires_grad_() for t in (x, *weights)]
    a_out, a_idx, a_losses = dense_fwd(*leaves)

    def dense_fwd_nograd():
        with torch.no_grad():
            return dense_fwd(x, *weights)

    levels = (8, 5, 5, 5)
    f_consts = ops.fsq_constants(levels, Q).to(dev)
    f_w = (torch.randn(4, dim, device=dev) * (1.5 / dim ** 0.5), torch.randn(4, device=dev) * 0.1, torch.randn(dim, 4, device=dev) * 0.5,
           torch.randn(dim, device=dev) * 0.1)
    f_z = ops.fsq_fwd(x, f_w, f_consts, 4, Q, k, idx.clone(), torch.empty_like(x), save_z=True)
    f_idx, f_out = torch.empty_like(idx), torch.empty_like(x)
    print(f'lfq [{M} x {dim}], {2 ** d} codes, Q {Q}: indices equal to the dense fp32 formulation on {float((a_idx == idx).all(dim=-1).float().mean()):.4%} '
          f'of the tokens, out rel-max {relerr(out, a_out.detach()):.2e}, losses rel-max {relerr(losses, a_losses.detach()):.2e}', flush=True)
    fns = [lambda: ops.lfq_fwd(x, weights, d, Q, k, idx, out, loss_cfg=cfg, ws=ws_f), dense_fwd_nograd,
           lambda: ops.fsq_fwd(x, f_w, f_consts, 4, Q, k, f_idx, f_out, save_z=True),
           lambda: ops.lfq_bwd(g, g_loss, x, z, avg, weights, d, Q, k, dx, cfg, ws=ws_b),
           lambda: torch.autograd.grad([a_out, a_losses], leaves, [g, g_loss], retain_graph=True),
           lambda: ops.fsq_bwd(g, x, f_z, f_w, f_consts, 4, Q, k, dx)]
    names = ('alm_lfq_fwd (3 launches)', 'dense torch fwd (no grad)', 'alm_fsq_fwd', 'alm_lfq_bwd (3 launches)', 'dense torch autograd bwd',
             'alm_fsq_bwd (2 launches)')
    for name, (med, lo, hi) in zip(names, median(fns)):
        print(f'  {name:28s} {med * 1e3:9.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})', flush=True)


def bench_gate_loop():
    """Gate-loop block (csrc/gate_loop.hip) at the default codec's eight stage shapes, batch and clip of the se_film section (8 x 10 s @ 16 kHz):
    after the encoder blocks C = 64 / 128 / 256 / 512 at T = 80000 / 20000 / 4000 / 500, after the decoder blocks C = 256 / 128 / 64 / 32 at
    T = 4000 / 20000 / 80000 / 160000 (five distinct shapes, each timed once).  Per shape: the two scan entry points alone with the rate on the bytes
    they move (forward 20 B per element: z 12, x, y; backward 28 B: g, q, a, h, dz 12), then the whole block, eval forward and training forward +
    backward, with the rate on the bytes the OP must move (forward 8 B per element: x in, y out; forward + backward 20 B: also g and x in, dx out)
    against the 6.29 TB/s copy rate of DESIGN section 20.  Then tokenize / decode of the default model without and with the layers.  Interleaved
    rounds, medians, one event pair per call.  Reported, not gated."""
    from audiolm_pytorch_amd import soundstream as S
    COPY = 6290.                                                  # GB/s

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(fns, rounds=7, warm=2):
        for _ in range(warm):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(rounds):
            for t, fn in zip(ts, fns):
                t.append(once(fn))
        return [sorted(t)[len(t) // 2] for t in ts]

    torch.manual_seed(0)
    B, n = 8, 160000
    stages = [('enc 1', 64, n // 2), ('enc 2', 128, n // 8), ('enc 3', 256, n // 40), ('enc 4', 512, n // 320),
              ('dec 1', 256, n // 40), ('dec 2', 128, n // 8), ('dec 3', 64, n // 2), ('dec 4', 32, n)]
    print(f'chunk {ops.GATE_LOOP_CHUNK}; {"stage":6s} {"shape":18s} {"scan fwd":>9s} {"GB/s":>6s} {"scan bwd":>9s} {"GB/s":>6s} | {"block fwd":>9s} {"GB/s":>6s} '
          f'{"of copy":>7s} | {"block f+b":>9s} {"GB/s":>6s} {"of copy":>7s}', flush=True)
    done = {}
    for name, C, T in stages:
        if (C, T) not in done:
            x, g = torch.randn(B, C, T, device=dev), torch.randn(B, C, T, device=dev)
            block = S.GateLoopBlock(C).to(dev)
            with torch.no_grad():
                z = block.launches(x)[0]
            h = ops.gate_loop_scan_fwd(z)
            xg = x.detach().requires_grad_()

            def fwd():
                with torch.no_grad():
                    return block.eval()(x)

            def step():
                block.train().zero_grad(set_to_none=True)
                xg.grad = None
                block(xg).backward(g)

            done[(C, T)] = median([lambda: ops.gate_loop_scan_fwd(z, x), lambda: ops.gate_loop_scan_bwd(g, z, h), fwd, step]) + [x.numel() / 1e6]
            del x, g, z, h, xg, block
        t_sf, t_sb, t_f, t_s, me = done[(C, T)]
        print(f'{"":11s}{name:6s} {f"C={C} T={T}":18s} {t_sf:9.3f} {20 * me / t_sf:6.0f} {t_sb:9.3f} {28 * me / t_sb:6.0f} | {t_f:9.3f} {8 * me / t_f:6.0f} '
              f'{8 * me / t_f / COPY:7.1%} | {t_s:9.3f} {20 * me / t_s:6.0f} {20 * me / t_s / COPY:7.1%}', flush=True)
    wave = torch.randn(B, n, device=dev) * 0.3
    gen = torch.Generator().manual_seed(5)
    rows = []
    for label, kw in (('without', {}), ('with gate-loop layers', dict(use_gate_loop_layers=True, with_gate_loop=True))):
        ss = A.SoundStream(codebook_size=1024, rq_num_quantizers=8, **kw)
        for layer in ss.rq.rvqs[0].layers:
            layer._codebook.embed.copy_(torch.randn(layer._codebook.embed.shape, generator=gen) * 0.5)
            layer._codebook.initted.fill_(True)
        ss.to(dev)
        codes = ss.tokenize(wave)

        def decode():
            with torch.no_grad():
                return ss.decode_from_codebook_indices(codes)

        rows.append((label, median([lambda: ss.tokenize(wave), decode], rounds=5)))
        del ss
    for label, (t_tok, t_dec) in rows:
        print(f'default SoundStream, {B} x {n} samples, {label:22s}: tokenize {t_tok:8.2f} ms   decode {t_dec:8.2f} ms', flush=True)


def bench_vqw2v():
    """native FairseqVQWav2Vec.forward at the released size (8 conv layers of 512 channels, 2 groups of 320 codes), 8 x 30 s at 16 kHz, against the
    plain-torch restatement (tests/vq_wav2vec_restated.py) in fp32 eager torch on the same GPU in the same process.  One event pair per forward,
    median of 20 after 3 warm-up runs; then the same for each native stage."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import vq_wav2vec_restated as VR
    sd = VR.random_state_dict(1)
    sd['vector_quantizer.embedding'] = torch.randn(320, 2, 256, generator=torch.Generator().manual_seed(2))
    m = A.FairseqVQWav2Vec.from_state_dict(sd, target_sample_hz=16000).to(dev)
    sdg = {k: v.to(dev) for k, v in sd.items()}
    wave = torch.randn(8, 480000, device=dev) * 0.3

    def median_ms(fn, iters=20, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]
    with torch.no_grad():
        nat = median_ms(lambda: m(wave))
        feat = median_ms(lambda: m.features(wave))
        ze = m.features(wave)
        asg = median_ms(lambda: m.assign(ze))
        ref = median_ms(lambda: VR.assign(VR.features(sdg, wave), sdg['vector_quantizer.embedding']), iters=5, warm=1)
        same = float((m(wave, flatten=False) == VR.assign(VR.features(sdg, wave), sdg['vector_quantizer.embedding'])).float().mean())
    w0 = sd['feature_extractor.conv_layers.0.0.weight'].view(512, 10).to(dev)
    g, b = sdg['feature_extractor.conv_layers.0.2.weight'], sdg['feature_extractor.conv_layers.0.2.bias']
    st0 = ops.vqw2v_conv0_stats(wave, w0, 5)
    x0 = ops.vqw2v_conv0_apply(wave, w0, st0, g, b, 5)
    x1 = ops.conv1d_valid(x0, sdg['feature_extractor.conv_layers.1.0.weight'], stride=4)
    st1 = ops.vqw2v_group_stats(x1, 1)
    gb = lambda t: t.numel() * 4 / 1e6                             # noqa: E731
    for name, fn, mb in (('conv0 stats', lambda: ops.vqw2v_conv0_stats(wave, w0, 5), gb(wave)),
                         ('conv0 apply', lambda: ops.vqw2v_conv0_apply(wave, w0, st0, g, b, 5), gb(wave) + gb(x0)),
                         ('conv layer 1 (512 -> 512, k 8, s 4)', lambda: ops.conv1d_valid(x0, sdg['feature_extractor.conv_layers.1.0.weight'], stride=4), gb(x0) + gb(x1)),
                         ('group stats layer 1', lambda: ops.vqw2v_group_stats(x1, 1), gb(x1)),
                         ('group apply layer 1 (in place)', lambda: ops.vqw2v_group_apply(x1, st1, g, b, relu=True), 2 * gb(x1))):
        t = median_ms(fn)
        print(f'  {name:38s} {t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})  {mb / t[0]:7.0f} GB/s', flush=True)
    print(f'vq-wav2vec released size 8 x 480000: native forward {nat[0]:.3f} ms (min {nat[1]:.3f}, max {nat[2]:.3f}; features {feat[0]:.3f}, assign {asg[0]:.3f})   '
          f'eager torch fp32 {ref[0]:.3f} ms (min {ref[1]:.3f}, max {ref[2]:.3f})   native / eager {nat[0] / ref[0]:.2f}   ids equal on {100 * same:.2f} %')


if __name__ == '__main__':
    what = sys.argv[1:] or ['gemm', 'attn', 'hc', 'misc']
    print(torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count)
    for w in what:
        globals()['bench_' + w]()
