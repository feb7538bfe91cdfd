"""Generates tests/golden/soundstream_losses_mel.pt: the generator loss of the REAL reference SoundStream (soundstream.py:927-995; imported under
oracle/ref_shims.py) WITH its multi-spectral mel-spectrogram reconstruction term at the reference defaults (six scales, weight 1e-5), on CPU.
Build-container only (the reference cannot travel); the fixture is committed.  Re-run:  python tests/golden/make_mel_loss_golden.py

torchaudio is not installed: before the reference module is constructed the stubbed `torchaudio.transforms.MelSpectrogram` is replaced by
tests/mel_restated.py's MelSpectrogramRestated (restated from torchaudio's published implementation, never compared against an installed torchaudio),
so the reference's OWN loss assembly (soundstream.py:938-945, :990) runs over it.

Modelled on make_stft_discr_golden.py: the same small CTOR but with the default mel settings and weight, the same wave (2 x 2560), the same seed
discipline (parameter VALUES re-synthesised from (shapes, seed) by tests/golden/common.py on both sides; the mel buffers keep their constructed values),
`ss.train(); ss.rq.eval()`, float64.

Stored: the five losses and the total; the grad_digest (norm taken in float64 + strided sample) of every `decoder.*` gradient of the total
(`gen_grads`) and of `multi_spectral_recon_loss.backward()` ALONE (`mel_grads`: at weight 1e-5 the mel share of the total's gradient is too small to
test); `fp32_deviation`: per stored key ('loss:<name>', 'gen:<key>', 'mel:<key>') the relative deviation of the SAME computation in fp32 on the CPU from
the float64 one (the floor of the GPU test's tolerance per key); the key -> shape list of `mel_spec_transforms.*`.

Margins asserted (else pick another SEED): every non-zero |Mo - Mr| of the mel term lies further from zero than KINK_FACTOR = 10 times its own fp32
deviation; every mel value is exactly 0 in both precisions or lies above the clamp's 1e-20 by the same factor; and, as in make_stft_discr_golden.py,
every ModReLU |z| + b, every |logit| of the STFT discriminator and every LeakyReLU pre-activation of the wave discriminators keeps that distance from
its kink."""
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
from mel_restated import MelSpectrogramRestated  # noqa: E402

warnings.filterwarnings('ignore')
torch.set_num_threads(1)                                     # one summation order for the fp32 run, whatever the machine
A, S, AT = ref_shims.load_reference()
S.T.MelSpectrogram = MelSpectrogramRestated                  # soundstream.py:15 `import torchaudio.transforms as T`; :662 `T.MelSpectrogram(...)`

SEED = 57
KINK_FACTOR = 10.
EPS = 1e-20
CTOR = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False)
PREFIXES = ('encoder.', 'decoder.', 'rq.', 'discriminators.', 'stft_discriminator.')
NAMES = ('recon', 'multi_spectral', 'adversarial', 'feature', 'commitment')


def wave_input():
    g = torch.Generator().manual_seed(43)
    return torch.randn(2, 2560, generator=g) * 0.3


def run(dtype):
    torch.manual_seed(0)
    ss = S.SoundStream(**CTOR)
    assert isinstance(ss.stft_discriminator, S.ComplexSTFTDiscriminator) and ss.multi_spectral_recon_loss_weight == 1e-5
    assert len(ss.mel_spec_transforms) == 6 and all(isinstance(t, MelSpectrogramRestated) for t in ss.mel_spec_transforms)
    full_sd = ss.state_dict()
    shapes = {k: tuple(v.shape) for k, v in full_sd.items() if k.startswith(PREFIXES)}
    mel_shapes = {k: tuple(v.shape) for k, v in full_sd.items() if k.startswith('mel_spec_transforms.')}
    full_sd.update(synth_state_dict(shapes, SEED))
    ss.load_state_dict(full_sd)
    ss.to(dtype)
    ss.train()
    ss.rq.eval()
    ss.rq.register_forward_hook(lambda _m, _i, out: (out[0].to(dtype), out[1], out[2].to(dtype)))
    wave = wave_input().to(dtype)
    modrelu, logits, mels = [], [], []
    hooks = [m.register_forward_pre_hook(lambda mod, inp: modrelu.append((inp[0].detach().abs() + mod.b.detach()).reshape(-1).double()))
             for m in ss.stft_discriminator.modules() if isinstance(m, S.ModReLU)]
    hooks.append(ss.stft_discriminator.final_conv.register_forward_hook(lambda _m, _i, out: logits.append(out.detach().abs().reshape(-1).double())))
    hooks.extend(t.register_forward_hook(lambda _m, _i, out: mels.append(out.detach().reshape(-1).double())) for t in ss.mel_spec_transforms)

    def decoder_grads():
        out = {k: p.grad.detach().clone() for k, p in ss.named_parameters() if k.startswith('decoder.')}
        ss.zero_grad(set_to_none=True)
        return out

    def gen_pass():
        total, breakdown = ss(wave, return_loss_breakdown=True)
        total.backward()
        return total, breakdown

    pre_gen, (total, breakdown) = leaky_inputs(ss.discriminators, gen_pass)
    assert len(mels) == 12                                       # per scale (orig, recon), in that order (soundstream.py:939)
    mel_orig, mel_recon = torch.cat(mels[0::2]), torch.cat(mels[1::2])
    gen_grads = decoder_grads()
    _, breakdown2 = ss(wave, return_loss_breakdown=True)
    breakdown2[1].backward()                                     # the mel term alone
    mel_grads = decoder_grads()
    for h in hooks:
        h.remove()
    losses = dict(total=total.detach().double(), **{n: torch.as_tensor(v).detach().double() for n, v in zip(NAMES, breakdown)})
    return dict(losses=losses, gen_grads=gen_grads, mel_grads=mel_grads, leaky=torch.cat([t.double().reshape(-1) for t in pre_gen]),
                modrelu=torch.cat(modrelu), logits=torch.cat(logits), mel_orig=mel_orig, mel_recon=mel_recon, shapes=shapes, mel_shapes=mel_shapes)


def grad_digest(grads):
    """common.grad_digest's format (norm + strided sample) with the norm taken in float64"""
    out = {}
    for k, gr in grads.items():
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
    for which, tag in (('gen_grads', 'gen'), ('mel_grads', 'mel')):
        d32, d64 = grad_digest(r32[which]), grad_digest(r64[which])
        for k, v in d64.items():
            dev[f'{tag}:{k}'] = max(rel(d32[k]['sample'], v['sample']), abs(d32[k]['norm'] - v['norm']) / max(v['norm'], 1e-30))
    return dev


def main():
    r64 = run(torch.float64)
    r32 = run(torch.float32)
    margins = {}
    for what in ('modrelu', 'logits', 'leaky'):
        v64, v32 = r64[what], r32[what].double()
        unsafe = int((v64.abs() <= KINK_FACTOR * (v32 - v64).abs()).sum())
        assert unsafe == 0, f'{unsafe} {what} values lie within {KINK_FACTOR} fp32 errors of their kink: choose another SEED'
        margins[what] = dict(count=v64.numel(), gap=float(v64.abs().min()))
    d64, d32 = r64['mel_orig'] - r64['mel_recon'], r32['mel_orig'] - r32['mel_recon']
    live = d64 != 0
    unsafe = int((d64[live].abs() <= KINK_FACTOR * (d32[live] - d64[live]).abs()).sum())
    assert unsafe == 0, f'{unsafe} mel differences lie within {KINK_FACTOR} fp32 errors of zero: choose another SEED'
    margins['mel_difference'] = dict(count=int(live.sum()), zeros=int((~live).sum()), gap=float(d64[live].abs().min()))
    for which in ('mel_orig', 'mel_recon'):
        v64, v32 = r64[which], r32[which]
        zero = (v64 == 0) & (v32 == 0)
        unsafe = int((~zero & (v64 - EPS <= KINK_FACTOR * (v32 - v64).abs())).sum())
        assert unsafe == 0, f'{unsafe} {which} values lie within {KINK_FACTOR} fp32 errors of the clamp at {EPS}: choose another SEED'
        margins[which] = dict(count=v64.numel(), zeros=int(zero.sum()), smallest=float(v64[~zero].min()))
    dev = deviations(r32, r64)
    gen, mel = grad_digest(r64['gen_grads']), grad_digest(r64['mel_grads'])
    assert all(v['norm'] > 0 for v in gen.values()) and all(v['norm'] > 0 for v in mel.values())
    out = dict(name='soundstream_losses_mel', kind='soundstream_losses', ctor=CTOR, shapes=r64['shapes'], seed=SEED, restated=False,
               inputs=dict(wave=wave_input()), outputs=dict(losses=r64['losses'], gen_grads=gen, mel_grads=mel),
               mel_spec_transforms_shapes=r64['mel_shapes'], margins=margins, fp32_deviation=dev)
    path = os.path.join(HERE, 'soundstream_losses_mel.pt')
    torch.save(out, path)
    worst = max(dev, key=dev.get)
    print(path, os.path.getsize(path), 'bytes; losses', {k: float(v) for k, v in r64['losses'].items()}, '; margins', margins,
          '; worst fp32-vs-float64 deviation', worst, dev[worst], '; losses', {k: v for k, v in dev.items() if k.startswith('loss:')})


if __name__ == '__main__':
    main()
