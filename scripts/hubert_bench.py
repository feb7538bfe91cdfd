"""Device time of audiolm_pytorch_amd.HubertWithKmeans (csrc/hubert.hip, csrc/dense_f32.hip) at 8 x 10 s and 8 x 30 s of 16 kHz audio, HuBERT-base, 9 layers, 500 centres:
per kernel and end to end, beside the restated module (tests/hubert_restated.py) in fp32 through ATen on the same GPU.  The two end-to-end runs alternate
inside one process (native, ATen, native, ...), so that both see the same clocks and the same neighbours.  For the conv and GEMM kernels the achieved
FLOP/s is given as a fraction of the fp32 matrix peak (157.3 TFLOP/s, v_mfma_f32_32x32x2_f32); operation counts come from the shapes.

usage: python scripts/hubert_bench.py [--iters 5] [--warmup 2] [--out profiles/<name>.log]
Times are medians of CUDA-event-timed calls after warm-up (device time: the events bracket launches only).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import audiolm_pytorch_amd as A  # noqa: E402
from audiolm_pytorch_amd import ops  # noqa: E402
import hubert_restated as HR  # noqa: E402

FP32_MATRIX = 157.3e12


def stages(m, wave):
    """the launches of HubertWithKmeans.features + assign, one (name, flop, thunk) at a time; each thunk returns the next activation"""
    p = dict(m.named_parameters())
    B, T = wave.shape
    c0, k0, s0 = m.conv_layers[0]
    w0 = p['feature_extractor.conv_layers.0.0.weight'].view(c0, k0)
    n = (T - k0) // s0 + 1
    st = {}

    def save(key, val):
        st[key] = val
        return val
    yield 'conv0_stats', 2 * B * c0 * n * k0, lambda x: (save('s', ops.hubert_conv0_stats(wave, w0, s0)), wave)[1]
    yield 'conv0_apply', 2 * B * c0 * n * k0, lambda x: ops.hubert_conv0_apply(wave, w0, st['s'], p['feature_extractor.conv_layers.0.2.weight'],
                                                                               p['feature_extractor.conv_layers.0.2.bias'], s0)
    cin = c0
    for i, (c, k, s) in enumerate(m.conv_layers[1:], 1):
        n = (n - k) // s + 1
        w = p[f'feature_extractor.conv_layers.{i}.0.weight']
        yield f'conv{i}_k{k}s{s}', 2 * B * c * n * cin * k, lambda x, w=w, s=s: ops.conv1d_valid(x, w, stride=s, gelu=True)
        cin = c
    D, H = m.dim, m.heads
    yield 'layernorm_bct_split', 0, lambda x: ops.layernorm_bct_split(x, p['layer_norm.weight'], p['layer_norm.bias'])
    yield 'post_extract_proj', 2 * B * n * cin * D, lambda x: ops.conv1d_valid(x, p['post_extract_proj.weight'].unsqueeze(-1), p['post_extract_proj.bias'])
    yield 'pos_conv', 2 * B * n * D * (D // m.conv_pos_groups) * m.conv_pos, lambda x: ops.conv1d_valid(
        x, m._pos_w, p['encoder.pos_conv.0.bias'], pad=m.conv_pos // 2, groups=m.conv_pos_groups, gelu=True, residual=x, drop_last=1 - m.conv_pos % 2)
    yield 'layernorm_bct_split', 0, lambda x: ops.layernorm_bct_split(x, p['encoder.layer_norm.weight'], p['encoder.layer_norm.bias'])
    for i in range(m.output_layer):
        pre = f'encoder.layers.{i}.'
        ffn = p[pre + 'fc1.weight'].shape[0]
        yield 'qkv_proj', 2 * B * n * D * 3 * D, lambda x, i=i: ops.conv1d_valid(save('x', x), getattr(m, f'_qkv_w{i}'), getattr(m, f'_qkv_b{i}'))
        yield 'mha_attn', 4 * B * n * n * D, lambda x: ops.mha_attn(x, H)
        yield 'out_proj', 2 * B * n * D * D, lambda x, pre=pre: ops.conv1d_valid(
            x, p[pre + 'self_attn.out_proj.weight'].unsqueeze(-1), p[pre + 'self_attn.out_proj.bias'], residual=st['x'])
        yield 'layernorm_bct_split', 0, lambda x, pre=pre: save('x', ops.layernorm_bct_split(
            x, p[pre + 'self_attn_layer_norm.weight'], p[pre + 'self_attn_layer_norm.bias']))
        yield 'fc1_gelu', 2 * B * n * D * ffn, lambda x, pre=pre: ops.conv1d_valid(x, p[pre + 'fc1.weight'].unsqueeze(-1), p[pre + 'fc1.bias'], gelu=True)
        yield 'fc2', 2 * B * n * D * ffn, lambda x, pre=pre: ops.conv1d_valid(
            x, p[pre + 'fc2.weight'].unsqueeze(-1), p[pre + 'fc2.bias'], residual=st['x'])
        yield 'layernorm_bct_split', 0, lambda x, pre=pre: ops.layernorm_bct_split(x, p[pre + 'final_layer_norm.weight'], p[pre + 'final_layer_norm.bias'])
    yield 'bct_to_btc', 0, lambda x: ops.bct_to_btc(x)
    yield 'kmeans_assign', 2 * B * n * D * m.codebook_size, lambda x: m.assign(x)


def per_kernel(m, wave, iters, warmup):
    acc = {}
    for it in range(warmup + iters):
        x = wave
        for name, flop, fn in stages(m, wave):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            x = fn(x)
            b.record()
            b.synchronize()
            if it >= warmup:
                e = acc.setdefault(name, dict(flop=0, us=[0.0] * iters, calls=0))
                e['us'][it - warmup] += a.elapsed_time(b) * 1e3
                if it == warmup:
                    e['flop'] += flop
                    e['calls'] += 1
    return x, {k: dict(calls=v['calls'], us=round(statistics.median(v['us']), 1), gflop=round(v['flop'] / 1e9, 2),
                       peak_fraction=round(v['flop'] / (statistics.median(v['us']) * 1e-6) / FP32_MATRIX, 3) if v['flop'] else None) for k, v in acc.items()}


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seconds', type=int, nargs='*', default=[10, 30])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'hubert_bench.py measures on the MI355X'
    dev = torch.device('cuda:0')
    sd = HR.random_state_dict(1, layers=9)
    centres = torch.randn(500, 768, generator=torch.Generator().manual_seed(2))
    m = A.HubertWithKmeans.from_state_dict(sd, centres).to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    cen_dev = centres.to(dev)
    lines = [f'# hubert_bench: HuBERT-base, 9 layers, 500 centres, fp32; median of {args.iters} event-timed runs after {args.warmup} warm-up runs '
             f'({torch.cuda.get_device_name(0)})']
    for secs in args.seconds:
        B, T = 8, secs * 16000
        wave = torch.randn(B, T, device=dev, generator=torch.Generator(device=dev).manual_seed(secs)) * 0.3

        def aten():
            with torch.no_grad():
                return HR.assign(HR.features(sd_dev, wave, 9, dtype=torch.float32), cen_dev)
        ids_k, table = per_kernel(m, wave, args.iters, args.warmup)
        nat, ref = [], []
        for it in range(args.warmup + args.iters):                      # interleaved: native, ATen, native, ATen, ...
            tn, tr = event_time(lambda: m(wave)), event_time(aten)
            if it >= args.warmup:
                nat.append(tn)
                ref.append(tr)
        ids_n, ids_a = m(wave), aten()
        flop = sum(v['gflop'] for v in table.values())
        r = dict(batch=B, seconds=secs, frames=int(ids_n.shape[1]), native_ms=round(statistics.median(nat), 2), native_min_max=[round(min(nat), 2), round(max(nat), 2)],
                 aten_fp32_ms=round(statistics.median(ref), 2), aten_min_max=[round(min(ref), 2), round(max(ref), 2)],
                 native_over_aten=round(statistics.median(nat) / statistics.median(ref), 3), gflop=round(flop, 1),
                 native_fraction_of_fp32_matrix_peak_end_to_end=round(flop * 1e9 / (statistics.median(nat) * 1e-3) / FP32_MATRIX, 3),
                 sum_of_kernels_ms=round(sum(v['us'] for v in table.values()) / 1e3, 2), ids_equal_to_aten=round(float((ids_n == ids_a).float().mean()), 4),
                 ids_equal_stagewise=bool(torch.equal(ids_k, ids_n)))
        lines.append(json.dumps(r))
        for k, v in table.items():
            lines.append(f'  {secs:2d} s  {k:18s} x{v["calls"]:<2d} {v["us"]:10.1f} us  {v["gflop"]:9.2f} GFLOP' +
                         (f'  {v["peak_fraction"]:.3f} of fp32 matrix peak' if v['peak_fraction'] is not None else ''))
        del wave
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
