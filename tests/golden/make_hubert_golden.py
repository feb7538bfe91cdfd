"""Writes tests/golden/hubert_tiny.pt and tests/golden/hubert_ref_forward.pt (CPU, needs `transformers`; the second file also needs the reference
checkout, loaded through oracle/ref_shims.py).  Run from the repository root:  python tests/golden/make_hubert_golden.py

hubert_tiny.pt        : a small HuBERT configuration, its seeded weights under fairseq's names, a wave, the features transformers.HubertModel computes
                        for it in fp64, and k-means centres.  Pins tests/hubert_restated.py where transformers is absent.
hubert_ref_forward.pt : token ids recorded from the REFERENCE's own HubertWithKmeans.forward (object made without its __init__, .model = the restated
                        network in fp64), for seq_len_multiple_of in (None, 320) and both values of flatten (weights and centres: hubert_tiny.pt).
                        Pins the order of operations, the cdist / argmax convention and the output shapes.  Only recorded data is stored.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

TINY = dict(dim=64, layers=2, heads=1, ffn=128, conv=[(32, 10, 5)] + [(32, 3, 2)] * 4 + [(32, 2, 2)] * 2, conv_pos=32, groups=16)


def hf_model(sd, layers, heads, ffn, conv, conv_pos, groups, dtype=torch.float64):
    """transformers.HubertModel (eval, no dropout / masking) carrying the fairseq-named weights `sd`"""
    from transformers import HubertConfig, HubertModel
    from audiolm_pytorch_amd.hubert_kmeans import fairseq_to_hf_state_dict
    dim = sd['post_extract_proj.weight'].shape[0]
    cfg = HubertConfig(hidden_size=dim, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn, hidden_act='gelu',
                       conv_dim=tuple(c for c, _, _ in conv), conv_kernel=tuple(k for _, k, _ in conv), conv_stride=tuple(s for _, _, s in conv),
                       conv_bias=False, feat_extract_norm='group', feat_extract_activation='gelu', feat_proj_layer_norm=True,
                       num_conv_pos_embeddings=conv_pos, num_conv_pos_embedding_groups=groups, do_stable_layer_norm=False, layer_norm_eps=1e-5,
                       hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0., final_dropout=0., layerdrop=0.,
                       apply_spec_augment=False, attn_implementation='eager')
    model = HubertModel(cfg).eval()
    want = set(model.state_dict())
    hf = fairseq_to_hf_state_dict({k: v for k, v in sd.items() if not k.startswith('encoder.layers.') or int(k.split('.')[2]) < layers})
    if 'encoder.pos_conv_embed.conv.weight_g' not in want:              # newer torch spells weight norm as a parametrization
        hf['encoder.pos_conv_embed.conv.parametrizations.weight.original0'] = hf.pop('encoder.pos_conv_embed.conv.weight_g')
        hf['encoder.pos_conv_embed.conv.parametrizations.weight.original1'] = hf.pop('encoder.pos_conv_embed.conv.weight_v')
    if 'masked_spec_embed' in want and 'masked_spec_embed' not in hf:
        hf['masked_spec_embed'] = model.state_dict()['masked_spec_embed']
    model.load_state_dict(hf, strict=True)
    return model.to(dtype)


def centres_from(sd, cfg, n_centres, seed, noise=0.05):
    """centres drawn from the fp64 features of other seeded clips plus small noise (so that real frames have a clearly nearest centre)"""
    import hubert_restated as HR
    g = torch.Generator().manual_seed(seed)
    clips = torch.randn(4, 16000, generator=g) * 0.3
    f = HR.features(sd, clips, cfg['layers'], cfg['heads'], cfg['conv'], cfg['groups'], torch.float64).reshape(-1, cfg['dim'])
    pick = torch.randperm(f.shape[0], generator=g)[:n_centres]
    return (f[pick] + noise * torch.randn(n_centres, cfg['dim'], generator=g, dtype=torch.float64)).float()


def main():
    import hubert_restated as HR
    cfg = TINY
    sd = HR.random_state_dict(11, cfg['dim'], cfg['layers'], cfg['ffn'], cfg['conv'], cfg['conv_pos'], cfg['groups'])
    g = torch.Generator().manual_seed(12)
    wave = torch.randn(2, 4000, generator=g) * 0.3
    model = hf_model(sd, cfg['layers'], cfg['heads'], cfg['ffn'], cfg['conv'], cfg['conv_pos'], cfg['groups'])
    with torch.no_grad():
        feats = model(wave.double()).last_hidden_state
    centres = centres_from(sd, cfg, 50, 13)
    torch.save({'config': cfg, 'state_dict': sd, 'wave': wave, 'hf_features64': feats, 'centres': centres}, os.path.join(HERE, 'hubert_tiny.pt'))
    print('hubert_tiny.pt', tuple(feats.shape))

    import ref_shims
    ref_shims.load_reference()
    import importlib
    import warnings
    import logging
    warn, level = warnings.warn, logging.root.level
    HK = importlib.import_module('audiolm_pytorch.hubert_kmeans')      # the reference module (it silences warnings / logging on import: restored)
    warnings.warn = warn
    logging.root.setLevel(level)
    wave2 = torch.randn(3, 5003, generator=g) * 0.3
    cases = []
    for mult in (None, 320):
        for flatten in (True, False):
            ref = HK.HubertWithKmeans.__new__(HK.HubertWithKmeans)
            torch.nn.Module.__init__(ref)
            ref.target_sample_hz, ref.seq_len_multiple_of, ref.output_layer = 16000, mult, cfg['layers']
            ref.model = HR.Model(sd, cfg['heads'], cfg['conv'], cfg['groups'], torch.float64)
            ref.register_buffer('cluster_centers', centres.double())
            ids = ref.forward(wave2, flatten=flatten)
            cases.append({'seq_len_multiple_of': mult, 'flatten': flatten, 'ids': ids.clone()})
            print('ref forward', mult, flatten, tuple(ids.shape))
    torch.save({'wave': wave2, 'cases': cases}, os.path.join(HERE, 'hubert_ref_forward.pt'))


if __name__ == '__main__':
    main()
