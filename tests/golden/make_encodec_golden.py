"""Writes tests/golden/encodec_tiny.pt and tests/golden/encodec_ref_forward.pt (CPU, needs `transformers`; the second file also needs the reference
checkout, loaded through oracle/ref_shims.py).  Run from the repository root:  python tests/golden/make_encodec_golden.py

encodec_tiny.pt        : a small EnCodec configuration, its seeded weights (biases included) under the transformers names, two waves (a multiple of the
                         hop and a ragged length) and what transformers.EncodecModel computes for them in fp64: encoder output, codes, decoded wave.
                         Pins tests/encodec_restated.py where transformers is absent.
encodec_ref_forward.pt : outputs recorded from the REFERENCE's own EncodecWrapper.forward / get_emb_from_indices / decode_from_codebook_indices (object
                         made without its __init__, .model = the restated adapter in fp64; weights: encodec_tiny.pt).  The shim's stub of Meta's
                         _linear_overlap_add is replaced by the restatement below.  Pins the order of operations, layouts and shapes.  Recorded data only.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

TINY = dict(num_filters=4, hidden_size=16, codebook_size=32, upsampling_ratios=[4, 2], num_lstm_layers=2)
BANDWIDTH = 60.0                       # 5 bits x 3000 frames / s per level: 4 levels


def hf_model(sd, cfg, dtype=torch.float64):
    from transformers import EncodecConfig, EncodecModel
    model = EncodecModel(EncodecConfig(target_bandwidths=[15., 30., BANDWIDTH], **cfg)).eval()
    own = model.state_dict()
    assert model.config.num_quantizers == 4 and not [k for k in sd if k not in own]
    model.load_state_dict(dict(own, **sd), strict=True)          # `own` supplies inited / cluster_size / embed_avg
    return model.to(dtype)


def linear_overlap_add(frames, stride):
    """Meta's encodec.utils._linear_overlap_add (the same routine as transformers' EncodecModel._linear_overlap_add): triangle-weighted overlap-add"""
    shape, dtype = frames[0].shape[:-1], frames[0].dtype
    total = stride * (len(frames) - 1) + frames[-1].shape[-1]
    n = frames[0].shape[-1]
    t = torch.linspace(0, 1, n + 2, dtype=dtype)[1:-1]
    weight = 0.5 - (t - 0.5).abs()
    sum_weight, out, offset = torch.zeros(total, dtype=dtype), torch.zeros(*shape, total, dtype=dtype), 0
    for frame in frames:
        m = frame.shape[-1]
        out[..., offset:offset + m] += weight[:m] * frame
        sum_weight[offset:offset + m] += weight[:m]
        offset += stride
    return out / sum_weight


def main():
    import encodec_restated as ER
    cfg = TINY
    sd = ER.random_state_dict(21, num_codebooks=4, **cfg)
    g = torch.Generator().manual_seed(22)
    waves = {'even': torch.randn(2, 320, generator=g) * 0.3, 'ragged': torch.randn(2, 331, generator=g) * 0.3}
    model = hf_model(sd, cfg)
    hf = {}
    with torch.no_grad():
        for name, wave in waves.items():
            feats = model.encoder(wave.double()[:, None])                              # [b, d, n]
            codes = model.quantizer.encode(feats, BANDWIDTH)                           # [q, b, n]
            audio = model.decoder(model.quantizer.decode(codes))                       # [b, 1, n * hop]
            hf[name] = {'features64': feats.transpose(1, 2).contiguous(), 'codes': codes.permute(1, 2, 0).contiguous(), 'decoded64': audio}
            print('encodec_tiny.pt', name, tuple(feats.shape), tuple(codes.shape), tuple(audio.shape))
    torch.save({'config': cfg, 'bandwidth': BANDWIDTH, 'state_dict': sd, 'waves': waves, 'hf': hf}, os.path.join(HERE, 'encodec_tiny.pt'))

    import ref_shims
    ref_shims.load_reference()
    import importlib
    ENC = importlib.import_module('audiolm_pytorch.encodec')           # the reference module
    ENC._linear_overlap_add = linear_overlap_add
    ref = ENC.EncodecWrapper.__new__(ENC.EncodecWrapper)
    torch.nn.Module.__init__(ref)
    ref.model = ER.Model(sd, BANDWIDTH, torch.float64, **cfg)
    ref.target_sample_hz, ref.codebook_dim, ref.rq_groups, ref.num_quantizers, ref.strides = 24000, cfg['hidden_size'], 1, ref.model.n_q, (2, 4)
    wave3, wave23 = torch.randn(3, 203, generator=g) * 0.3, torch.randn(2, 3, 96, generator=g) * 0.3
    rec = {'wave3': wave3, 'wave23': wave23}
    emb, codes, none = ref.forward(wave3.double(), return_encoded=True)
    assert none is None
    rec['encoded'] = {'emb': emb.clone(), 'codes': codes.clone()}
    emb0, codes0, _ = ref.forward(wave3.double())
    assert emb0 is None and torch.equal(codes0, codes)
    rec['codes_only'] = codes0.clone()
    emb23, codes23, _ = ref.forward(wave23.double(), return_encoded=True)
    rec['lead_dims'] = {'emb': emb23.clone(), 'codes': codes23.clone()}
    rec['get_emb_from_indices'] = ref.get_emb_from_indices(codes).clone()
    rec['decode_b1'] = ref.decode_from_codebook_indices(codes[:1]).clone()
    rec['decode_emb'] = ref.decode(emb[:1]).clone()
    rec['seq_len_multiple_of'] = ref.seq_len_multiple_of
    for k, v in rec.items():
        print('encodec_ref_forward.pt', k, {n: (tuple(t.shape), t.dtype) for n, t in v.items()} if isinstance(v, dict) else getattr(v, 'shape', v))
    torch.save(rec, os.path.join(HERE, 'encodec_ref_forward.pt'))


if __name__ == '__main__':
    main()
