"""Device time of audiolm_pytorch_amd.resample (csrc/resample.hip) at 8 x 30 s clips, 16 / 44.1 / 48 kHz -> 24 kHz, forward and adjoint, each beside
its floor max(bytes / 6.29 TB/s, 2 T outputs / 157 TFLOP/s) (HBM rate and fp32 vector peak of the MI355X), and the SoundStream tokenize time of the
same clips at 24 kHz (BASELINE config 5 codec shape), so that the resampler's share of the tokenize path is visible.

usage: python scripts/resample_bench.py [--iters 30] [--warmup 5] [--out profiles/<name>.log]
Times are medians of CUDA-event-timed single calls after warm-up (device time: no host work inside the events).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import audiolm_pytorch_amd as A  # noqa: E402
from audiolm_pytorch_amd import ops  # noqa: E402
import importlib  # noqa: E402

RS = importlib.import_module('audiolm_pytorch_amd.resample')
HBM, FP32 = 6.29e12, 157e12


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'resample_bench.py measures on the MI355X'
    dev = torch.device('cuda:0')
    lines = [f'# resample_bench: 8 x 30 s clips -> 24 kHz, median of {args.iters} event-timed calls after {args.warmup} warm-up calls ({torch.cuda.get_device_name(0)})']
    B, secs, new = 8, 30, 24000
    results = []
    for orig in (16000, 44100, 48000):
        o, n, W, T = RS.geometry(orig, new)
        L = secs * orig
        Lout = RS.output_length(L, orig, new)
        x = torch.randn(B, L, device=dev, generator=torch.Generator(device=dev).manual_seed(orig))
        dy = torch.randn(B, Lout, device=dev, generator=torch.Generator(device=dev).manual_seed(orig + 1))
        table = RS._device_table(dev, orig, new, 6, 0.99, 'sinc_interp_hann', None)
        nbytes = (B * L + B * Lout + n * T) * 4
        floor = max(nbytes / HBM, 2 * T * B * Lout / FP32) * 1e6
        fwd = timed(lambda: ops.resample_sinc(x, table, o, n, W), args.iters, args.warmup)
        bwd = timed(lambda: ops.resample_sinc_bwd(dy, table, L, o, n, W), args.iters, args.warmup)
        r = dict(orig=orig, new=new, o=o, n=n, W=W, T=T, bytes=nbytes, floor_us=round(floor, 2), fwd_us=round(fwd[0], 2), fwd_min_max=[round(fwd[1], 2), round(fwd[2], 2)],
                 bwd_us=round(bwd[0], 2), bwd_min_max=[round(bwd[1], 2), round(bwd[2], 2)], fwd_x_floor=round(fwd[0] / floor, 2), bwd_x_floor=round(bwd[0] / floor, 2))
        results.append(r)
        lines.append(json.dumps(r))
        del x, dy
    torch.manual_seed(0)
    ss = A.SoundStream(codebook_size=4096, rq_num_quantizers=8, target_sample_hz=24000, strides=(2, 4, 5, 8), use_local_attn=False).to(dev)
    with torch.no_grad():                                   # a trained codec's codebooks stand in as scaled random ones (as in scripts/conv_bench.py)
        for r in ss.rq.rvqs:
            for q, l in enumerate(r.layers):
                l._codebook.embed.copy_(torch.randn(1, 4096, 512) * (0.5 ** q))
                l._codebook.initted.fill_(True)
    w24 = torch.randn(B, secs * new, device=dev) * 0.3
    tok = timed(lambda: ss.tokenize(w24), max(5, args.iters // 3), 2)
    lines.append(json.dumps(dict(tokenize_24k_8x30s_us=round(tok[0], 1), tokenize_min_max=[round(tok[1], 1), round(tok[2], 1)])))
    for r in results:
        lines.append(f"{r['orig']} -> {new}: fwd {r['fwd_us']} us ({r['fwd_x_floor']}x floor {r['floor_us']} us), bwd {r['bwd_us']} us "
                     f"({r['bwd_x_floor']}x), resample fwd = {100 * r['fwd_us'] / (r['fwd_us'] + tok[0]):.1f} % of resample + tokenize")
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
