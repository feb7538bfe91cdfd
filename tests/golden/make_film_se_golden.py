"""Generates tests/golden/film_se_small.pt: losses, reconstructions and every gradient of the REAL reference SoundStream's conv stacks with
squeeze_excite=True and its two FiLM conditioners (first-party code, soundstream.py:145-169, 332-395, 442-449; imported under oracle/ref_shims.py like
make_codec_bwd_golden.py does) on CPU in fp32.  Build-container only (the reference cannot travel); the fixture is committed.
Re-run:  python tests/golden/make_film_se_golden.py

    cond = [is_denoising, not is_denoising]
    y = decoder(decoder_film(encoder_film(encoder(x)^T, cond), cond)^T)        no quantiser in between
    loss = mse(y, x)

for is_denoising = True and False (each `to_cond.weight` gradient has one zero column per condition, so both are stored).  Parameter VALUES are
re-synthesised from (shapes, seed) by tests/golden/common.py on both sides; the fixture stores the wave and per condition the loss, the reconstruction
and the gradient of every `encoder.*` / `decoder.*` / `encoder_film.*` / `decoder_film.*` parameter, packed into ONE flat tensor per condition
(`grad_flat` + `grad_index` rows (name, shape, stride, offset, count); tests/film_se_restated.py golden_grads unpacks them).  161145 gradient elements
per condition are 645 KB, two full sets would pass the 1 MiB limit of a committed file: is_denoising=True is stored in full, is_denoising=False in
full for every tensor of up to 4096 elements (all FiLM and squeeze-excite parameters, all biases) and as every 8th element of the larger conv weights.
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

SEED = 23
PREFIXES = ('encoder.', 'decoder.', 'encoder_film.', 'decoder_film.')


def pack(grads, full_up_to=None):
    index, chunks, off = [], [], 0
    for k in sorted(grads):
        flat = grads[k].reshape(-1)
        stride = 1 if full_up_to is None or flat.numel() <= full_up_to else 8
        part = flat[::stride].clone()
        index.append((k, tuple(grads[k].shape), stride, off, part.numel()))
        chunks.append(part)
        off += part.numel()
    return torch.cat(chunks), index


def main():
    torch.manual_seed(0)
    ctor = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, strides=(2, 4, 5, 8), use_local_attn=False, squeeze_excite=True)
    ss = S.SoundStream(**ctor)
    full_sd = ss.state_dict()
    keep = {k: v for k, v in full_sd.items() if k.startswith(PREFIXES)}
    shapes = {k: tuple(v.shape) for k, v in keep.items()}
    full_sd.update(synth_state_dict(shapes, SEED))
    ss.load_state_dict(full_sd)
    ss.train()
    g = torch.Generator().manual_seed(33)
    wave = torch.randn(2, 320 * 12 + 77, generator=g) * 0.3
    x, _ = ss.process_input(wave)                                # (b, 1, n) curtailed to a multiple of 320
    outputs = {}
    for is_denoising in (True, False):
        ss.zero_grad(set_to_none=True)
        cond = torch.tensor([is_denoising, not is_denoising], dtype=x.dtype)
        f = ss.encoder(x).transpose(1, 2)
        f = ss.decoder_film(ss.encoder_film(f, cond), cond)
        y = ss.decoder(f.transpose(1, 2))
        loss = F.mse_loss(y, x)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in ss.named_parameters() if k.startswith(PREFIXES)}
        assert all(v is not None and torch.isfinite(v).all() for v in grads.values())
        assert all(float(v.abs().max()) > 0 for v in grads.values()), [k for k, v in grads.items() if float(v.abs().max()) == 0]
        flat, index = pack(grads, None if is_denoising else 4096)
        outputs['denoise' if is_denoising else 'plain'] = dict(loss=loss.detach().clone(), recon=y.detach().clone(), grad_flat=flat, grad_index=index)
    out = dict(name='film_se_small', kind='film_se', ctor=ctor, shapes=shapes, seed=SEED, restated=False, inputs=dict(wave=wave), outputs=outputs)
    path = os.path.join(HERE, 'film_se_small.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes; losses', float(outputs['denoise']['loss']), float(outputs['plain']['loss']), '; grads', len(grads))


if __name__ == '__main__':
    main()
