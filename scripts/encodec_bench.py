"""EncodecWrapper at the 24 kHz geometry on the MI355X: encode and decode milliseconds for 8 x 30 s (override with --batch / --seconds), split into
convolutions, LSTM (with its launch count) and RVQ.  Seeded random weights (speed does not depend on their values).

Timing: device events around each stage after a warm-up, the median of --reps repetitions; the split is taken by timing the LSTM and the RVQ on their
own with the tensors they see in the model, the convolutions are the remainder.  Run from the repository root:  python scripts/encodec_bench.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--seconds', type=float, default=30.)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()

    import audiolm_pytorch_amd as A
    from audiolm_pytorch_amd import encodec as ENC, ops
    import encodec_restated as ER
    dev = torch.device('cuda:0')
    sd = ER.random_state_dict(1, zero_bias=True)
    m = A.EncodecWrapper.from_state_dict(sd).to(dev)
    T = int(args.seconds * 24000)
    wave = (torch.randn(args.batch, T, generator=torch.Generator().manual_seed(2)) * 0.3).to(dev)
    n = -(-T // 320)

    feats = m.encode(wave)
    codes = m.quantize(feats)
    emb = m.get_emb_from_indices(codes)
    images = m._prepare()
    enc_lstm = next(k for k in images if k.startswith('encoder.') and k.endswith('.lstm'))
    dec_lstm = next(k for k in images if k.startswith('decoder.') and k.endswith('.lstm'))
    x = torch.randn(args.batch, 512, n, device=dev) * 0.3

    r = {'batch': args.batch, 'seconds': args.seconds, 'frames': n, 'num_quantizers': m.num_quantizers,
         'lstm_launches': ops.lstm_launches(n, m.config['num_lstm_layers'])}
    r['encode_ms'] = timed(lambda: m(wave), args.reps)
    r['encode_lstm_ms'] = timed(lambda: ENC.lstm_skip(images[enc_lstm], x), args.reps)
    r['encode_rvq_ms'] = timed(lambda: m.quantize(feats), args.reps)
    r['encode_conv_ms'] = r['encode_ms'] - r['encode_lstm_ms'] - r['encode_rvq_ms']
    r['decode_ms'] = timed(lambda: m.decode_from_codebook_indices(codes), args.reps)
    r['decode_lstm_ms'] = timed(lambda: ENC.lstm_skip(images[dec_lstm], x), args.reps)
    r['decode_rvq_ms'] = timed(lambda: m.get_emb_from_indices(codes), args.reps)
    r['decode_conv_ms'] = r['decode_ms'] - r['decode_lstm_ms'] - r['decode_rvq_ms']
    r['lstm_us_per_launch'] = 1e3 * r['encode_lstm_ms'] / r['lstm_launches']
    print(f"encode {r['encode_ms']:.1f} ms = conv {r['encode_conv_ms']:.1f} + lstm {r['encode_lstm_ms']:.1f} ({r['lstm_launches']} launches, "
          f"{r['lstm_us_per_launch']:.1f} us each) + rvq {r['encode_rvq_ms']:.1f}")
    print(f"decode {r['decode_ms']:.1f} ms = conv {r['decode_conv_ms']:.1f} + lstm {r['decode_lstm_ms']:.1f} + rvq lookup {r['decode_rvq_ms']:.1f}")
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in r.items()}))
    assert emb.shape == (args.batch, n, 128)


if __name__ == '__main__':
    main()
