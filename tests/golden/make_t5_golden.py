"""Writes tests/golden/t5_tiny.pt: forwards recorded from the real transformers.T5EncoderModel in fp64 on the CPU (needs `transformers`; run by hand,
never by the tests).

  python tests/golden/make_t5_golden.py

The file holds, for a tiny gated-gelu config and a tiny relu config: the config, the state dict (fp32 values; the model is run on their fp64 images),
ids, ragged attention masks (a full row, a one-token row, a prefix row and a non-prefix row) and the zero-masked outputs as reference t5.py:94-110
forms them; and the indices T5Attention._relative_position_bucket gives for every key - query in -600 .. 600, for (num_buckets, max_distance) =
(32, 128) and (16, 40).

One thing is changed in the recorded model: transformers' T5LayerNorm takes its variance in fp32 whatever the module's dtype
(`hidden_states.to(torch.float32).pow(2).mean(-1)`, a guard for half-precision weights), which would leave fp32 rounding (1e-7) in an otherwise
fp64 forward.  fp64_norms() gives the real model's norm modules the same formula without the cast, so that the recording is an fp64 yardstick
throughout; attention, position bias, buckets, masking, feed-forward and the module wiring are transformers' own code.  `output_unpatched` is the
same forward of the model exactly as transformers ships it (norms included), for a check of the norm that owes nothing to this file.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import t5_restated as TR  # noqa: E402

CONFIGS = {
    'gated': dict(d_model=64, num_heads=2, d_kv=64, d_ff=64, num_layers=2, vocab_size=50, feed_forward_proj='gated-gelu',
                  relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6),
    'relu': dict(d_model=32, num_heads=1, d_kv=64, d_ff=64, num_layers=2, vocab_size=50, feed_forward_proj='relu',
                 relative_attention_num_buckets=16, relative_attention_max_distance=40, layer_norm_epsilon=1e-6),
}


def fp64_norms(model):
    import types
    from transformers.models.t5.modeling_t5 import T5LayerNorm

    def forward(self, hidden_states):                      # T5LayerNorm.forward without the .to(torch.float32) of the variance
        variance = hidden_states.pow(2).mean(-1, keepdim=True)
        return self.weight * (hidden_states * torch.rsqrt(variance + self.variance_epsilon))
    norms = [m for m in model.modules() if isinstance(m, T5LayerNorm)]
    assert len(norms) == 2 * model.config.num_layers + 1, 'the norm modules are not transformers.T5LayerNorm (a fused replacement?)'
    for m in norms:
        m.forward = types.MethodType(forward, m)
    return model


def hf_model(sd, cfg, patch_norms=True):
    from transformers import T5Config, T5EncoderModel
    model = T5EncoderModel(T5Config(**cfg, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)).double().eval()
    if patch_norms:
        model = fp64_norms(model)
    full = {k: v.double() for k, v in sd.items()}
    full['encoder.embed_tokens.weight'] = full['shared.weight']
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and not [k for k in missing if k not in full], (missing, unexpected)
    return model


def main():
    from transformers.models.t5.modeling_t5 import T5Attention
    out = {}
    T = 40
    g = torch.Generator().manual_seed(7)
    mask = torch.ones(4, T, dtype=torch.long)
    mask[1, 1:] = 0
    mask[2, 17:] = 0
    mask[3, 5:9] = 0
    mask[3, 30:] = 0
    for seed, (name, cfg) in enumerate(CONFIGS.items()):
        sd = TR.random_state_dict(seed + 1, d_model=cfg['d_model'], layers=cfg['num_layers'], heads=cfg['num_heads'], d_ff=cfg['d_ff'],
                                  vocab=cfg['vocab_size'], gated=cfg['feed_forward_proj'] == 'gated-gelu',
                                  num_buckets=cfg['relative_attention_num_buckets'])
        ids = torch.randint(0, cfg['vocab_size'], (4, T), generator=g)
        with torch.no_grad():
            hidden = hf_model(sd, cfg)(input_ids=ids, attention_mask=mask).last_hidden_state
            untouched = hf_model(sd, cfg, patch_norms=False)(input_ids=ids, attention_mask=mask).last_hidden_state
        out[name] = dict(config=cfg, state_dict=sd, ids=ids, mask=mask, output64=hidden.masked_fill(~mask[..., None].bool(), 0.),
                         output_unpatched=untouched.masked_fill(~mask[..., None].bool(), 0.))
    delta = torch.arange(-600, 601)
    out['delta'] = delta
    out['buckets'] = {f'{nb},{md}': T5Attention._relative_position_bucket(delta, bidirectional=True, num_buckets=nb, max_distance=md).to(torch.int16)
                      for nb, md in ((32, 128), (16, 40))}
    path = os.path.join(HERE, 't5_tiny.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
