"""Plain-torch restatements for the discriminator tests (test infrastructure; any dtype, CPU).

`MultiScaleDiscriminatorRestated` states the reference's MultiScaleDiscriminator (soundstream.py:92-140: first-party code, a handful of nn.Conv1d) with
the same module tree, so `state_dict()` keys are interchangeable with the package's module.  `TinyWaveDiscriminator` is the small caller-supplied
`stft_discriminator` of the end-to-end fixture: tests/golden/make_discr_golden.py hands THIS class to the real reference and the GPU test hands it to
the package, so both sides run the identical module.  `discr_loss` / `generator_losses` compose the loss branches (soundstream.py:868-995) from such pieces.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn


class MultiScaleDiscriminatorRestated(nn.Module):
    def __init__(self, channels=16, layers=4, groups=(4, 16, 64, 256), chan_max=1024, input_channels=1):
        super().__init__()
        self.init_conv = nn.Conv1d(input_channels, channels, 15, padding=7)
        self.conv_layers = nn.ModuleList([])
        curr = channels
        for _, group in zip(range(layers), groups):
            out = min(curr * 4, chan_max)
            self.conv_layers.append(nn.Sequential(nn.Conv1d(curr, out, 41, stride=4, padding=20, groups=group), nn.LeakyReLU(0.1)))
            curr = out
        self.final_conv = nn.Sequential(nn.Conv1d(curr, curr, 5, padding=2), nn.LeakyReLU(0.1), nn.Conv1d(curr, 1, 3, padding=1))

    def forward(self, x, return_intermediates=False):
        x = self.init_conv(x)
        inter = []
        for layer in self.conv_layers:
            x = layer(x)
            inter.append(x)
        out = self.final_conv(x)
        return (out, inter) if return_intermediates else out


class TinyWaveDiscriminator(nn.Module):
    """stand-in for an STFT discriminator: three small convs on the wave, `forward(x, return_intermediates=False)` like the reference's"""

    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([nn.Sequential(nn.Conv1d(1, 4, 9, stride=4, padding=4), nn.LeakyReLU(0.1)),
                                     nn.Sequential(nn.Conv1d(4, 8, 9, stride=4, padding=4), nn.LeakyReLU(0.1))])
        self.out = nn.Conv1d(8, 1, 3, padding=1)

    def forward(self, x, return_intermediates=False):
        inter = []
        for layer in self.layers:
            x = layer(x)
            inter.append(x)
        out = self.out(x)
        return (out, inter) if return_intermediates else out


def leaky_inputs(module, run):
    """(the input of every nn.LeakyReLU inside `module`, in call order, while `run()` executes; run()'s result)"""
    seen = []
    hooks = [m.register_forward_pre_hook(lambda _, inp: seen.append(inp[0].detach().clone())) for m in module.modules() if isinstance(m, nn.LeakyReLU)]
    try:
        out = run()
    finally:
        for h in hooks:
            h.remove()
    return seen, out


def min_leaky_gap(module, run):
    """smallest |pre-activation| any nn.LeakyReLU inside `module` sees while `run()` executes"""
    seen, out = leaky_inputs(module, run)
    return min(float(t.abs().min()) for t in seen), out


def hinge_discr_loss(fake, real):
    return (F.relu(1 + fake) + F.relu(1 - real)).mean()


def downsample(x, f):
    return x if f is None else F.avg_pool1d(x, 2 * f, stride=f, padding=f)


def discr_loss(discrs, factors, stft, real, fake):
    """soundstream.py:870-909: (mean over scales (+ stft term), [per-scale losses], stft loss | None); factors: None for the first scale"""
    stft_loss = None if stft is None else hinge_discr_loss(stft(fake), stft(real))
    losses = []
    for d, f in zip(discrs, factors):
        real, fake = downsample(real, f), downsample(fake, f)
        losses.append(hinge_discr_loss(d(fake), d(real)))
    total = torch.stack(losses).mean()
    return (total if stft_loss is None else total + stft_loss), losses, stft_loss


def generator_losses(discrs, factors, stft, real, fake, target=None):
    """soundstream.py:927-984 without the mel term: (recon, adversarial, feature)"""
    recon = F.mse_loss(real if target is None else target, fake)
    adv, pairs = [], []
    if stft is not None:
        _, ri = stft(real, return_intermediates=True)
        stft_fake, fi = stft(fake, return_intermediates=True)
        pairs.extend(zip(ri, fi))
    for d, f in zip(discrs, factors):
        real, fake = downsample(real, f), downsample(fake, f)
        _, ri = d(real, return_intermediates=True)
        fl, fi = d(fake, return_intermediates=True)
        adv.append(-fl.mean())
        pairs.extend(zip(ri, fi))
    feature = torch.stack([F.l1_loss(r, f) for r, f in pairs]).mean()
    if stft is not None:
        adv.append(-stft_fake.mean())
    return recon, torch.stack(adv).mean(), feature
