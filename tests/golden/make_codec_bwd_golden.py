"""Generates tests/golden/codec_bwd_small.pt: loss and every encoder / decoder gradient of the REAL reference SoundStream's conv stacks (first-party
code, soundstream.py:332-395, 519-531, 615-627; imported under oracle/ref_shims.py like make_golden.py does) on CPU in fp32.  Build-container only
(the reference cannot travel); the fixture is committed.  Re-run:  python tests/golden/make_codec_bwd_golden.py

    y = decoder(encoder(x))        no quantiser in between ('b c n -> b n c' and back cancel)
    loss = mse(y, x)

Parameter VALUES are re-synthesised from (shapes, seed) by tests/golden/common.py on both sides; the fixture stores the wave, the loss and the full
gradient of every `encoder.*` / `decoder.*` parameter (a few tens of KB).
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

SEED = 21


def main():
    torch.manual_seed(0)
    ctor = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, strides=(2, 4, 5, 8), use_local_attn=False)
    ss = S.SoundStream(**ctor)
    full_sd = ss.state_dict()
    keep = {k: v for k, v in full_sd.items() if k.startswith(('encoder.', 'decoder.', 'rq.'))}
    shapes = {k: tuple(v.shape) for k, v in keep.items()}
    full_sd.update(synth_state_dict(shapes, SEED))
    ss.load_state_dict(full_sd)
    ss.train()
    g = torch.Generator().manual_seed(31)
    wave = torch.randn(2, 320 * 12 + 77, generator=g) * 0.3
    x, _ = ss.process_input(wave)                                # (b, 1, n) curtailed to a multiple of 320
    y = ss.decoder(ss.encoder(x))
    loss = F.mse_loss(y, x)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in ss.named_parameters() if k.startswith(('encoder.', 'decoder.'))}
    assert all(v is not None and torch.isfinite(v).all() for v in grads.values())
    out = dict(name='codec_bwd_small', kind='codec_bwd', ctor=ctor, shapes=shapes, seed=SEED, restated=False, inputs=dict(wave=wave),
               outputs=dict(loss=loss.detach().clone(), recon=y.detach().clone(), grads=grads))
    path = os.path.join(HERE, 'codec_bwd_small.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes; loss', float(loss), '; grads', len(grads))


if __name__ == '__main__':
    main()
