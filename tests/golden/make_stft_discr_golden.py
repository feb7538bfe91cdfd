"""Generates tests/golden/soundstream_losses_stft.pt: the loss branches of the REAL reference SoundStream (soundstream.py:868-995; imported under
oracle/ref_shims.py) with its DEFAULT ComplexSTFTDiscriminator, on CPU.  Build-container only (the reference cannot travel); the fixture is committed.
Re-run:  python tests/golden/make_stft_discr_golden.py

Modelled on make_discr_golden.py: the same small CTOR, the same wave (2 x 2560), the same seed discipline (parameter VALUES re-synthesised from
(shapes, seed) by tests/golden/common.py on both sides; ModReLU's b comes out non-zero), `ss.train(); ss.rq.eval()`, a generator pass with
return_loss_breakdown=True, a discriminator pass, and the `separately` list, all in float64.

Stored: the losses; the grad_digest (norm taken in float64 + strided sample) of every `decoder.*`, `discriminators.*` and `stft_discriminator.*`
gradient of both passes; the `stft_discriminator.*` key -> shape list; `fp32_deviation`: per stored key ('loss:<name>', 'separately:<name>',
'gen:<key>', 'discr:<key>') the relative deviation of the SAME computation in fp32 on the CPU from the float64 one (the floor of the GPU test's
tolerance per key); `init_sums`: per-parameter float64 sums of the reference module's initial values under torch.manual_seed(0).

Margins asserted (else pick another SEED): every ModReLU |z| + b, every |logit| of the STFT discriminator, every |a - b| of its feature term and every
LeakyReLU pre-activation of the wave discriminators lies further from zero than KINK_FACTOR = 10 times its own deviation in the fp32 run -- an fp32
evaluation must not land on the other side of a kink (see make_discr_golden.py for why an absolute margin cannot be kept at this size)."""
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
GRAD_PREFIXES = ('decoder.', 'discriminators.', 'stft_discriminator.')


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
    modrelu, logits, feature = [], [], []
    hooks = [m.register_forward_pre_hook(lambda mod, inp: modrelu.append((inp[0].detach().abs() + mod.b.detach()).reshape(-1).double()))
             for m in ss.stft_discriminator.modules() if isinstance(m, S.ModReLU)]
    hooks.append(ss.stft_discriminator.final_conv.register_forward_hook(lambda _m, _i, out: logits.append(out.detach().abs().reshape(-1).double())))
    calls = []
    hooks.append(ss.stft_discriminator.register_forward_hook(lambda _m, _i, out: calls.append(out)))

    def grads():
        out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in ss.named_parameters() if k.startswith(GRAD_PREFIXES)}
        ss.zero_grad(set_to_none=True)
        return out

    def gen_pass():
        total, breakdown = ss(wave, return_loss_breakdown=True)
        total.backward()
        return total, breakdown

    pre_gen, (total, breakdown) = leaky_inputs(ss.discriminators, gen_pass)
    (_, real_inter), (_, fake_inter) = calls                    # the generator pass: (real, fake), each with its intermediates
    feature = [(a.detach() - b.detach()).abs().reshape(-1).double() for a, b in zip(real_inter, fake_inter)]
    gen_grads = grads()

    def discr_pass():
        loss = ss(wave, return_discr_loss=True)
        loss.backward()
        return loss

    pre_discr, discr = leaky_inputs(ss.discriminators, discr_pass)
    discr_grads = grads()
    with torch.no_grad():
        separately = ss(wave, return_discr_loss=True, return_discr_losses_separately=True)
    for h in hooks:
        h.remove()
    names = ('recon', 'multi_spectral', 'adversarial', 'feature', 'commitment')
    losses = dict(total=total.detach().double(), discr=discr.detach().double(),
                  **{n: torch.as_tensor(v).detach().double() for n, v in zip(names, breakdown)})
    return dict(losses=losses, separately=[(n, v.detach().double()) for n, v in separately], gen_grads=gen_grads, discr_grads=discr_grads,
                leaky=torch.cat([t.double().reshape(-1) for t in pre_gen + pre_discr]), modrelu=torch.cat(modrelu), logits=torch.cat(logits),
                feature=torch.cat(feature), shapes=shapes)


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


def deviations(r32, r64):
    dev = {}
    for k, v in r64['losses'].items():
        dev[f'loss:{k}'] = rel(r32['losses'][k], v) if float(v) != 0. else 0.
    for (n, a), (_, b) in zip(r32['separately'], r64['separately']):
        dev[f'separately:{n}'] = rel(a, b)
    for which, tag in (('gen_grads', 'gen'), ('discr_grads', 'discr')):
        d32, d64 = grad_digest(r32[which]), grad_digest(r64[which])
        for k, v in d64.items():
            if v is None:
                assert d32[k] is None, k
                continue
            dev[f'{tag}:{k}'] = max(rel(d32[k]['sample'], v['sample']), abs(d32[k]['norm'] - v['norm']) / max(v['norm'], 1e-30))
    return dev


def init_sums():
    torch.manual_seed(0)
    m = S.ComplexSTFTDiscriminator()
    return {k: float(v.double().sum()) for k, v in m.state_dict().items()}


def main():
    r64 = run(torch.float64)
    r32 = run(torch.float32)
    margins = {}
    for what in ('modrelu', 'logits', 'feature', 'leaky'):
        v64, v32 = r64[what], r32[what].double()
        unsafe = int((v64.abs() <= KINK_FACTOR * (v32 - v64).abs()).sum())
        assert unsafe == 0, f'{unsafe} {what} values lie within {KINK_FACTOR} fp32 errors of their kink: choose another SEED'
        margins[what] = dict(count=v64.numel(), gap=float(v64.abs().min()))
    dev = deviations(r32, r64)
    assert [n for n, _ in r64['separately']] == ['scale:1', 'scale:0.5', 'scale:0.25', 'stft']
    gen, dis = grad_digest(r64['gen_grads']), grad_digest(r64['discr_grads'])
    assert all(v is not None for v in gen.values())
    assert all((v is None) == k.startswith('decoder.') for k, v in dis.items())
    out = dict(name='soundstream_losses_stft', kind='soundstream_losses', ctor=CTOR, shapes=r64['shapes'], seed=SEED, restated=False,
               inputs=dict(wave=wave_input()),
               outputs=dict(losses=r64['losses'], separately=r64['separately'], gen_grads=gen, discr_grads=dis),
               stft_discriminator_shapes={k: s for k, s in r64['shapes'].items() if k.startswith('stft_discriminator.')},
               margins=margins, fp32_deviation=dev, init_sums=init_sums())
    path = os.path.join(HERE, 'soundstream_losses_stft.pt')
    torch.save(out, path)
    worst = max(dev, key=dev.get)
    print(path, os.path.getsize(path), 'bytes; losses', {k: float(v) for k, v in r64['losses'].items()}, '; separately',
          [(n, float(v)) for n, v in r64['separately']], '; margins', margins, '; worst fp32-vs-float64 deviation', worst, dev[worst],
          '; losses', {k: v for k, v in dev.items() if k.startswith(('loss:', 'separately:'))})


if __name__ == '__main__':
    main()
