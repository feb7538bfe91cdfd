"""Generates tests/golden/codec_bwd_local_attn_small.pt: loss and every encoder / encoder_attn / decoder_attn / decoder gradient of the REAL reference
SoundStream in its DEFAULT form (use_local_attn=True, soundstream.py:545, 613, 830-833, 705-709) on CPU in fp32, imported under oracle/ref_shims.py
with the restated local-attention modules (oracle/local_attention_restated.py) as its `local_attention` stub -> restated=True.  Build-container only
(the reference cannot travel); the fixture is committed.  Re-run:  python tests/golden/make_local_attn_bwd_golden.py

    h = encoder_attn(rearrange(encoder(x), 'b c n -> b n c'))          no quantiser in between
    y = decoder(rearrange(decoder_attn(h), 'b n c -> b c n'))
    loss = mse(y, x)

The constructor is that of soundstream_local_attn_small.pt (window 64, 2 heads x 32, depth 2); 70 frames = one full window and a ragged second one.
Parameter VALUES are re-synthesised from (shapes, seed) by tests/golden/common.py on both sides (the rotary inv_freq buffers keep their constructor
values: const_keys); the fixture stores the wave (fp16: the samples are rounded to
fp16 before the reference runs, so the stored tensor is the exact input), the loss and the full fp32 gradient of every parameter of the four stacks.
"""
from __future__ import annotations

import os
import sys
import warnings

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402
from common import synth_state_dict  # noqa: E402

warnings.filterwarnings('ignore')
A, S, AT = ref_shims.load_reference()

SEED = 8
STACKS = ('encoder', 'encoder_attn', 'decoder_attn', 'decoder')


def main():
    torch.manual_seed(0)
    ctor = dict(codebook_size=32, rq_num_quantizers=4, channels=4, codebook_dim=16, strides=(2, 4, 5, 8), target_sample_hz=16000,
                attn_window_size=64, attn_dim_head=32, attn_heads=2, attn_depth=2)
    ss = S.SoundStream(**ctor)
    full_sd = ss.state_dict()
    keep = {k: v for k, v in full_sd.items() if k.split('.')[0] in STACKS + ('rq',)}
    shapes = {k: tuple(v.shape) for k, v in keep.items()}
    new = synth_state_dict(shapes, SEED)
    const_keys = [k for k in shapes if k.endswith('rel_pos.inv_freq')]
    for k in const_keys:
        new[k] = full_sd[k].clone()                              # the rotary frequencies are a constant buffer, not a parameter
    full_sd.update(new)
    ss.load_state_dict(full_sd)
    ss.train()
    g = torch.Generator().manual_seed(41)
    wave = (torch.randn(2, 320 * 70 + 31, generator=g) * 0.3).half()     # fp16-representable samples: stored as fp16, the exact input of both sides
    wave16, wave = wave, wave.float()
    x, _ = ss.process_input(wave)                                # (b, 1, n) curtailed to a multiple of 320
    h = ss.encoder_attn(ss.encoder(x).transpose(1, 2))
    y = ss.decoder(ss.decoder_attn(h).transpose(1, 2))
    loss = F.mse_loss(y, x)
    loss.backward()
    named = [(k, p.grad.detach()) for k, p in ss.named_parameters() if k.split('.')[0] in STACKS]
    flat = torch.cat([v.reshape(-1) for _, v in named])          # one storage, the gradients are views of it: one record in the file instead of 168
    grads, off = {}, 0
    for k, v in named:
        grads[k] = flat[off:off + v.numel()].view(v.shape)
        off += v.numel()
    assert all(v is not None and torch.isfinite(v).all() and v.abs().max() > 0 for v in grads.values())
    out = dict(name='codec_bwd_local_attn_small', kind='codec_bwd_local_attn', ctor=ctor, shapes=shapes, seed=SEED, restated=True, const_keys=const_keys,
               inputs=dict(wave=wave16), outputs=dict(loss=loss.detach().clone(), grads=grads))
    path = os.path.join(HERE, 'codec_bwd_local_attn_small.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes; loss', float(loss), '; grads', len(grads))


if __name__ == '__main__':
    main()
