"""Plain-torch restatement of the reference's gradient penalty (soundstream.py:70-83) and of the discriminator loss branch that uses it
(soundstream.py:870-925), written from their definition for the tests (test infrastructure; any dtype, CPU).  The discriminators are the restated
modules of tests/discr_restated.py and tests/stft_discr_restated.py.

gradient_penalty(wave, output, weight, center) = weight * mean_b (|G_b|_2 - center)^2 with G = d output / d wave taken with create_graph=True and
the norm per batch row over everything else.  The branch: the STFT discriminator's penalty is real + fake and joins the total; every wave
discriminator's (real, fake) pair goes to one flat list, which the package then zips with the SCALES, so the labels pair the scales with the first
len(scales) entries of that list ('scale_grad_penalty:0.5' is the fake penalty at scale 1)."""
from __future__ import annotations

import torch

from discr_restated import downsample, hinge_discr_loss


def gradient_penalty(wave, output, weight=10, center=0.):
    gradients, = torch.autograd.grad(outputs=output, inputs=wave, grad_outputs=torch.ones_like(output), create_graph=True)
    norms = torch.linalg.vector_norm(gradients.reshape(gradients.shape[0], -1), dim=1)       # subgradient 0 for an all-zero row
    return weight * ((norms - center) ** 2).mean()


def discr_losses_with_penalty(discrs, factors, scales, stft, real, fake, package=True):
    """(total, package) of the reference's discriminator branch with apply_grad_penalty=True; factors: None for the first scale; stft: a module
    or None.  package=False leaves out the wave discriminators' penalties, which do not reach the total (the package then has no
    'scale_grad_penalty:*' entries)"""
    stft_loss = stft_penalty = None
    if stft is not None:
        r, f = real.detach().clone().requires_grad_(), fake.detach().clone().requires_grad_()
        stft_loss = hinge_discr_loss(stft(f), stft(r))
        stft_penalty = gradient_penalty(r, stft_loss) + gradient_penalty(f, stft_loss)
    losses, penalties = [], []
    for d, factor in zip(discrs, factors):
        real, fake = downsample(real, factor).detach(), downsample(fake, factor).detach()
        r, f = real.clone().requires_grad_(), fake.clone().requires_grad_()
        loss = hinge_discr_loss(d(f), d(r))
        losses.append(loss)
        if package:
            penalties.extend([gradient_penalty(r, loss), gradient_penalty(f, loss)])
    total = torch.stack(losses).mean()
    if stft_loss is not None:
        total = total + stft_loss + stft_penalty
    package = [(f'scale:{s}', v) for s, v in zip(scales, losses)]
    package.extend((f'scale_grad_penalty:{s}', v) for s, v in zip(scales, penalties))
    if stft_loss is not None:
        package.extend([('stft', stft_loss), ('stft_grad_penalty', stft_penalty)])
    return total, package
