"""Generates tests/golden/soundstream_losses_small.pt: the loss branches of the REAL reference SoundStream (soundstream.py:868-995; imported under
oracle/ref_shims.py like make_codec_bwd_golden.py does) on CPU.  Build-container only (the reference cannot travel); the fixture is committed.
Re-run:  python tests/golden/make_discr_golden.py

    ss = SoundStream(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False, multi_spectral_recon_loss_weight=0.,
                     stft_discriminator=TinyWaveDiscriminator())          # tests/discr_restated.py: the same class the GPU test hands to the package
    ss.train(); ss.rq.eval()                                              # deterministic quantiser
    total, (recon, multi_spectral, adversarial, feature, commitment) = ss(wave, return_loss_breakdown=True);  total.backward()
    discr = ss(wave, return_discr_loss=True);  discr.backward()           # and once more with return_discr_losses_separately=True

Parameter VALUES are re-synthesised from (shapes, seed) by tests/golden/common.py on both sides.  Stored, from the float64 run: the losses and the
grad_digest (norm + strided sample) of every `decoder.*`, `discriminators.*` and `stft_discriminator.*` gradient of both backward passes, the
`discriminators.*` key -> shape list, and `fp32_deviation`: the largest relative deviation of the SAME computation in fp32 on the CPU from the float64
one, over every stored number (the floor of the GPU test's tolerance).

The LeakyReLU kink.  An absolute margin of 1e-5 around zero cannot be kept at this size by any choice of seed: one pass puts 1,041,920 pre-activations
of spread 0.06 .. 3 through the LeakyReLUs of the three default discriminators and the stand-in, so about 40 of them fall within 1e-5 of zero whatever
the seed (SEED 41: 42 of them, the nearest 2.0e-7 away; with the wave 10 / 100 / 1000 times louder still 13 / 9 / 7, from the reconstruction's side,
whose level the codebooks fix).  What the margin is there for is that an fp32 evaluation must not land on the other side of the kink, so the maker
asserts THAT, against the measured fp32 error: every float64 pre-activation is further from zero than KINK_FACTOR = 10 times its own deviation in the
fp32 run (the factor allows for another summation order, as in the tolerance), else pick another SEED.  The count within 1e-5 and the smallest
|pre-activation| are stored (`leaky_near`, `leaky_gap`).
"""
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
from discr_restated import TinyWaveDiscriminator, leaky_inputs  # noqa: E402

warnings.filterwarnings('ignore')
torch.set_num_threads(1)                                     # one summation order for the fp32 run, whatever the machine
A, S, AT = ref_shims.load_reference()

SEED = 57
GAP = 1e-5
KINK_FACTOR = 10.
CTOR = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False, multi_spectral_recon_loss_weight=0.)
PREFIXES = ('encoder.', 'decoder.', 'rq.', 'discriminators.', 'stft_discriminator.')
GRAD_PREFIXES = ('decoder.', 'discriminators.', 'stft_discriminator.')


def wave_input():
    g = torch.Generator().manual_seed(43)
    return torch.randn(2, 2560, generator=g) * 0.3


def run(dtype):
    torch.manual_seed(0)
    ss = S.SoundStream(**CTOR, stft_discriminator=TinyWaveDiscriminator())
    full_sd = ss.state_dict()
    shapes = {k: tuple(v.shape) for k, v in full_sd.items() if k.startswith(PREFIXES)}
    full_sd.update(synth_state_dict(shapes, SEED))
    ss.load_state_dict(full_sd)
    ss.to(dtype)
    ss.train()
    ss.rq.eval()
    # the restated eval-mode quantiser computes in fp32 whatever it is given (the synthesised codebooks are fp32 values: nothing is lost)
    ss.rq.register_forward_hook(lambda _m, _i, out: (out[0].to(dtype), out[1], out[2].to(dtype)))
    wave = wave_input().to(dtype)
    watched = torch.nn.ModuleList([ss.discriminators, ss.stft_discriminator])

    def grads():
        out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in ss.named_parameters() if k.startswith(GRAD_PREFIXES)}
        ss.zero_grad(set_to_none=True)
        return out

    def gen_pass():
        total, breakdown = ss(wave, return_loss_breakdown=True)
        total.backward()
        return total, breakdown

    pre_gen, (total, breakdown) = leaky_inputs(watched, gen_pass)
    gen_grads = grads()

    def discr_pass():
        loss = ss(wave, return_discr_loss=True)
        loss.backward()
        return loss

    pre_discr, discr = leaky_inputs(watched, discr_pass)
    discr_grads = grads()
    with torch.no_grad():
        separately = ss(wave, return_discr_loss=True, return_discr_losses_separately=True)
    names = ('recon', 'multi_spectral', 'adversarial', 'feature', 'commitment')
    losses = dict(total=total.detach().double(), discr=discr.detach().double(),
                  **{n: torch.as_tensor(v).detach().double() for n, v in zip(names, breakdown)})
    return dict(losses=losses, separately=[(n, v.detach().double()) for n, v in separately], gen_grads=gen_grads, discr_grads=discr_grads,
                pre=[t.double().reshape(-1) for t in pre_gen + pre_discr], shapes=shapes)


def grad_digest(grads, full=False):
    """common.grad_digest's format (norm + strided sample) with the norm taken in float64: the fp32 norm of the 5.2 M-element `final_conv.0.weight`
    gradients carries a summation error of 4e-4, twenty times the tolerance"""
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


def deviation(r32, r64):
    worst = 0.
    for k, v in r64['losses'].items():
        if float(v) != 0.:
            worst = max(worst, rel(r32['losses'][k], v))
    for (_, a), (_, b) in zip(r32['separately'], r64['separately']):
        worst = max(worst, rel(a, b))
    for which in ('gen_grads', 'discr_grads'):
        d32, d64 = grad_digest(r32[which], full=False), grad_digest(r64[which], full=False)
        for k, v in d64.items():
            if v is None:
                assert d32[k] is None, k
                continue
            worst = max(worst, rel(d32[k]['sample'], v['sample']), abs(d32[k]['norm'] - v['norm']) / max(v['norm'], 1e-30))
    return worst


def main():
    r64 = run(torch.float64)
    r32 = run(torch.float32)
    pre64, pre32 = torch.cat(r64['pre']), torch.cat(r32['pre'])
    unsafe = int((pre64.abs() <= KINK_FACTOR * (pre32 - pre64).abs()).sum())
    assert unsafe == 0, f'{unsafe} LeakyReLU pre-activations lie within {KINK_FACTOR} fp32 errors of zero: choose another SEED'
    gap, near = float(pre64.abs().min()), int((pre64.abs() < GAP).sum()) // 2          # both passes see the same values
    dev = deviation(r32, r64)
    assert [n for n, _ in r64['separately']] == ['scale:1', 'scale:0.5', 'scale:0.25', 'stft']
    gen, dis = grad_digest(r64['gen_grads'], full=False), grad_digest(r64['discr_grads'], full=False)
    assert all(v is not None for v in gen.values())
    assert all((v is None) == k.startswith('decoder.') for k, v in dis.items())          # the discriminator step sees the detached reconstruction
    out = dict(name='soundstream_losses_small', kind='soundstream_losses', ctor=CTOR, shapes=r64['shapes'], seed=SEED, restated=False,
               inputs=dict(wave=wave_input()),
               outputs=dict(losses=r64['losses'], separately=r64['separately'], gen_grads=gen, discr_grads=dis),
               discriminator_shapes={k: s for k, s in r64['shapes'].items() if k.startswith('discriminators.')},
               leaky_gap=gap, leaky_near=near, fp32_deviation=dev)
    path = os.path.join(HERE, 'soundstream_losses_small.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes; losses', {k: float(v) for k, v in r64['losses'].items()}, '; leaky gap', gap, 'near', near, 'of', pre64.numel() // 2,
          '; fp32-vs-float64 deviation', dev)


if __name__ == '__main__':
    main()
