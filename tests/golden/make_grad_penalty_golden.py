"""Generates tests/golden/soundstream_grad_penalty.pt: the discriminator branch of the REAL reference SoundStream with `apply_grad_penalty=True`
(soundstream.py:70-83, :870-925; imported under oracle/ref_shims.py) and its DEFAULT ComplexSTFTDiscriminator, on CPU.  Build-container only (the
reference cannot travel); the fixture is committed.  Re-run:  python tests/golden/make_grad_penalty_golden.py

Modelled on make_stft_discr_golden.py: the same small CTOR, the same wave (2 x 2560), parameter VALUES re-synthesised from (shapes, seed) by
tests/golden/common.py on both sides, `ss.train(); ss.rq.eval()`, in float64.

Stored from the float64 run: the eight-entry package (`return_discr_losses_separately=True`) in the reference's order; per entry the grad_digest
(float64 norm + strided sample) of every `discriminators.*` / `stft_discriminator.*` gradient after that entry's own `backward(retain_graph=True)`
(gradients zeroed between entries, as a trainer that steps per entry would see them); the non-separate total and its digests; `fp32_deviation`: per
stored key ('separately:<name>', 'entry:<name>:<param>', 'loss:total', 'total:<param>') the relative deviation of the SAME computation in fp32 on the
CPU from the float64 one (the floor of the GPU test's tolerance per key).

Margins asserted (else pick another SEED): every LeakyReLU pre-activation of the wave discriminators, every ModReLU |z| + b and every |logit| of the
STFT discriminator lies further from zero than KINK_FACTOR = 10 times its own deviation in the fp32 run, and every per-row gradient norm that enters
a penalty is non-zero.  SEED 57 (the seed of make_stft_discr_golden.py) passes."""
from __future__ import annotations

import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402
from common import synth_state_dict  # noqa: E402
from discr_restated import leaky_inputs  # noqa: E402

warnings.filterwarnings('ignore')
torch.set_num_threads(1)                                     # one summation order for the fp32 run, whatever the machine
A, S, AT = ref_shims.load_reference()

SEED = 57
KINK_FACTOR = 10.
CTOR = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False, multi_spectral_recon_loss_weight=0.)
PREFIXES = ('encoder.', 'decoder.', 'rq.', 'discriminators.', 'stft_discriminator.')
GRAD_PREFIXES = ('discriminators.', 'stft_discriminator.')
NAMES = ['scale:1', 'scale:0.5', 'scale:0.25', 'scale_grad_penalty:1', 'scale_grad_penalty:0.5', 'scale_grad_penalty:0.25', 'stft',
         'stft_grad_penalty']


def wave_input():
    g = torch.Generator().manual_seed(43)
    return torch.randn(2, 2560, generator=g) * 0.3


def run(dtype):
    torch.manual_seed(0)
    ss = S.SoundStream(**CTOR)
    assert isinstance(ss.stft_discriminator, S.ComplexSTFTDiscriminator)
    full_sd = ss.state_dict()
    shapes = {k: tuple(v.shape) for k, v in full_sd.items() if k.startswith(PREFIXES)}
    full_sd.update(synth_state_dict(shapes, SEED))
    ss.load_state_dict(full_sd)
    ss.to(dtype)
    ss.train()
    ss.rq.eval()
    ss.rq.register_forward_hook(lambda _m, _i, out: (out[0].to(dtype), out[1], out[2].to(dtype)))
    wave = wave_input().to(dtype)
    modrelu, logits, row_norms = [], [], []
    hooks = [m.register_forward_pre_hook(lambda mod, inp: modrelu.append((inp[0].detach().abs() + mod.b.detach()).reshape(-1).double()))
             for m in ss.stft_discriminator.modules() if isinstance(m, S.ModReLU)]
    hooks.append(ss.stft_discriminator.final_conv.register_forward_hook(lambda _m, _i, out: logits.append(out.detach().abs().reshape(-1).double())))
    torch_grad = S.torch_grad

    def recording_grad(*args, **kwargs):                     # the gradients that enter a penalty: their per-row norms, for the margin check
        out = torch_grad(*args, **kwargs)
        row_norms.append(out[0].detach().double().reshape(out[0].shape[0], -1).norm(dim=1))
        return out

    S.torch_grad = recording_grad

    def grads():
        out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in ss.named_parameters() if k.startswith(GRAD_PREFIXES)}
        ss.zero_grad(set_to_none=True)
        return out

    def separate_pass():
        pkg = ss(wave, return_discr_loss=True, return_discr_losses_separately=True, apply_grad_penalty=True)
        per_entry = {}
        for name, loss in pkg:                               # the trainer: one backward(retain_graph=True) per entry
            loss.backward(retain_graph=True)
            per_entry[name] = grads()
        return pkg, per_entry

    def total_pass():
        loss = ss(wave, return_discr_loss=True, apply_grad_penalty=True)
        loss.backward()
        return loss

    try:
        pre_sep, (pkg, per_entry) = leaky_inputs(ss.discriminators, separate_pass)
        pre_tot, total = leaky_inputs(ss.discriminators, total_pass)
        total_grads = grads()
    finally:
        S.torch_grad = torch_grad
        for h in hooks:
            h.remove()
    return dict(separately=[(n, v.detach().double()) for n, v in pkg], per_entry=per_entry, total=total.detach().double(), total_grads=total_grads,
                leaky=torch.cat([t.double().reshape(-1) for t in pre_sep + pre_tot]), modrelu=torch.cat(modrelu), logits=torch.cat(logits),
                row_norms=torch.cat(row_norms), shapes=shapes)


def grad_digest(grads):
    """common.grad_digest's format (norm + strided sample) with the norm taken in float64"""
    out = {}
    for k, gr in grads.items():
        if gr is None:
            out[k] = None
            continue
        flat = gr.detach().double().reshape(-1)
        stride = max(1, flat.numel() // 257)
        out[k] = dict(norm=float(flat.norm()), sample=flat[::stride].float().clone(), stride=stride, full=None)
    return out


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def digest_deviation(d32, d64, tag, dev):
    for k, v in d64.items():
        if v is None:
            assert d32[k] is None, (tag, k)
            continue
        if v['norm'] == 0.:
            assert d32[k]['norm'] == 0., (tag, k)
            dev[f'{tag}:{k}'] = 0.
            continue
        dev[f'{tag}:{k}'] = max(rel(d32[k]['sample'], v['sample']), abs(d32[k]['norm'] - v['norm']) / v['norm'])


def main():
    r64 = run(torch.float64)
    r32 = run(torch.float32)
    assert [n for n, _ in r64['separately']] == NAMES, [n for n, _ in r64['separately']]
    margins = {}
    for what in ('modrelu', 'logits', 'leaky'):
        v64, v32 = r64[what], r32[what].double()
        unsafe = int((v64.abs() <= KINK_FACTOR * (v32 - v64).abs()).sum())
        assert unsafe == 0, f'{unsafe} {what} values lie within {KINK_FACTOR} fp32 errors of their kink: choose another SEED'
        margins[what] = dict(count=v64.numel(), gap=float(v64.abs().min()))
    assert float(r64['row_norms'].min()) > 0. and float(r32['row_norms'].min()) > 0., 'a per-row gradient norm is zero: choose another SEED'
    margins['row_norms'] = dict(count=r64['row_norms'].numel(), gap=float(r64['row_norms'].min()))
    dev = {'loss:total': rel(r32['total'], r64['total'])}
    for (n, a), (_, b) in zip(r32['separately'], r64['separately']):
        dev[f'separately:{n}'] = rel(a, b)
    entries = {}
    for name in NAMES:
        entries[name] = grad_digest(r64['per_entry'][name])
        digest_deviation(grad_digest(r32['per_entry'][name]), entries[name], f'entry:{name}', dev)
    total_digest = grad_digest(r64['total_grads'])
    digest_deviation(grad_digest(r32['total_grads']), total_digest, 'total', dev)
    touched = {n: sum(1 for v in d.values() if v is not None) for n, d in entries.items()}
    out = dict(name='soundstream_grad_penalty', kind='soundstream_losses', ctor=CTOR, shapes=r64['shapes'], seed=SEED, restated=False,
               inputs=dict(wave=wave_input()),
               outputs=dict(separately=r64['separately'], entry_grads=entries, total=r64['total'], total_grads=total_digest),
               margins=margins, fp32_deviation=dev)
    path = os.path.join(HERE, 'soundstream_grad_penalty.pt')
    torch.save(out, path)
    worst = max(dev, key=dev.get)
    print(path, os.path.getsize(path), 'bytes; separately', [(n, float(v)) for n, v in r64['separately']], '; total', float(r64['total']),
          '; parameters touched per entry', touched, '; margins', margins, '; worst fp32-vs-float64 deviation', worst, dev[worst],
          '; losses', {k: v for k, v in dev.items() if k.startswith(('loss:', 'separately:'))})


if __name__ == '__main__':
    main()
