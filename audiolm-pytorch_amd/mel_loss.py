"""Multi-spectral mel-spectrogram reconstruction loss of SoundStream training (reference soundstream.py:645-672 and :933-945, eq. (4) / (5) of the
SoundStream paper) on the fp32 kernels of csrc/mel_loss.hip.

`MelSpectrogram` restates the subset of `torchaudio.transforms.MelSpectrogram` the reference uses, from torchaudio's published definition (torchaudio
is not a dependency): power 2, periodic Hann window zero-padded centred to n_fft, center=True with reflect padding, one-sided, HTK mel scale without
area normalisation, `normalized=True` dividing the spectrum by sqrt(sum(window^2)).  It keeps torchaudio's two persistent buffers under torchaudio's
names, `spectrogram.window` (win_length,) and `mel_scale.fb` (n_fft // 2 + 1, n_mels), so the `mel_spec_transforms.*` entries of a reference checkpoint
load.  The windowed DFT basis the kernels multiply by is derived from `window` (ops.stft_basis, float64 on the host, rounded once) and is NOT
persistent: it is rebuilt when the buffer changes (load_state_dict, .to(device)), found out by the buffer's version counter and address -- the device
buffer is read back only then, never per call.

`multi_spectral_recon_loss` runs real and fake waves of every scale as one batch [real | fake]; the gradient goes to the reconstruction only.
Per scale the forward is 4 launches (DFT product with |.|^2 in the epilogue, mel projection, per-frame norms, the sum's second stage) and the
backward 4 (the column gradient, fb x dMel with dX = 2 X dP in the epilogue, the two launches of the STFT backward).  Results are bitwise reproducible.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import ops
from .discriminators import _f32c, _needs_graph

F32 = torch.float32


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, dtype=torch.float64):
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale='htk'): triangular filters [n_freqs, n_mels]"""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_min, m_max = 2595. * math.log10(1. + f_min / 700.), 2595. * math.log10(1. + f_max / 700.)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype)
    f_pts = 700. * (10 ** (m_pts / 2595.) - 1.)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.)


class _Buffer(nn.Module):
    """a child that only holds one persistent buffer (torchaudio's Spectrogram.window / MelScale.fb key names)"""

    def __init__(self, name, value):
        super().__init__()
        self.register_buffer(name, value)


class _MelSpecFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module):
        mel, X, basis = module._mel(x, x_from=0)
        ctx.cfg = (x.shape[1], module.n_fft, module.hop_length)
        ctx.basis = basis
        ctx.save_for_backward(X, module.mel_scale.fb)
        return mel

    @staticmethod
    def backward(ctx, g):
        X, fb = ctx.saved_tensors
        n, n_fft, hop = ctx.cfg
        dX = ops.mel_power_bwd(g.to(F32).contiguous(), fb, X)
        return ops.stft_bwd(dX, ctx.basis, n, n_fft, hop), None


class _MelLossFn(torch.autograd.Function):
    """one scale of the loss: `both` = [real | fake] (no graph), `fake` the differentiable second half of it"""

    @staticmethod
    def forward(ctx, fake, both, module, alpha):
        mel, X, basis = module._mel(both, x_from=fake.shape[0])
        loss, _, norms = ops.mel_frame_loss(mel, alpha)
        ctx.cfg = (fake.shape[1], module.n_fft, module.hop_length, alpha)
        ctx.basis = basis
        ctx.save_for_backward(mel, norms, X, module.mel_scale.fb)
        return loss

    @staticmethod
    def backward(ctx, g):
        mel, norms, X, fb = ctx.saved_tensors
        n, n_fft, hop, alpha = ctx.cfg
        dmel = ops.mel_frame_loss_bwd(mel, norms, g.to(F32).contiguous(), alpha)
        dX = ops.mel_power_bwd(dmel, fb, X)
        return ops.stft_bwd(dX, ctx.basis, n, n_fft, hop), None, None, None


class MelSpectrogram(nn.Module):
    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, n_mels=128, normalized=False, **unsupported):
        super().__init__()
        if unsupported:
            raise NotImplementedError(f'MelSpectrogram: {", ".join(sorted(unsupported))} not implemented (fixed at torchaudio\'s defaults: f_min=0, '
                                      "f_max=sample_rate/2, power=2, Hann window, center=True, pad_mode='reflect', onesided, norm=None, mel_scale='htk')")
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        if not (0 < win_length <= n_fft and hop_length > 0 and n_mels > 0 and sample_rate > 0):
            raise ValueError(f'MelSpectrogram: need 0 < win_length <= n_fft, hop_length > 0, n_mels > 0 (got n_fft = {n_fft}, win_length = {win_length}, '
                             f'hop_length = {hop_length}, n_mels = {n_mels})')
        self.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels = sample_rate, n_fft, win_length, hop_length, n_mels
        self.normalized = bool(normalized)
        self.spectrogram = _Buffer('window', torch.hann_window(win_length, dtype=torch.float64).to(F32))
        self.mel_scale = _Buffer('fb', melscale_fbanks(n_fft // 2 + 1, 0., float(sample_rate // 2), n_mels, sample_rate).to(F32))
        self._basis_key = self._basis = None

    def _window(self, dtype=torch.float64):
        """the buffer's current values on the host, divided by sqrt(sum(window^2)) when normalized"""
        w = self.spectrogram.window.detach().to('cpu', dtype)
        return w / w.pow(2).sum().sqrt() if self.normalized else w

    def padded_window(self, dtype=torch.float64):
        """the window as the DFT sees it: zero-padded centred to n_fft (left pad (n_fft - win_length) // 2, like torch.stft)"""
        left = (self.n_fft - self.win_length) // 2
        return torch.nn.functional.pad(self._window(dtype), (left, self.n_fft - self.win_length - left))

    def _dft_basis(self, device):
        w = self.spectrogram.window
        key = (w._version, w.data_ptr(), str(w.device), str(device))
        if key != self._basis_key:                               # the only read-back of the device buffer: after construction, a load or a move
            self._basis = ops.stft_basis(self.n_fft, self._window(), False, device)
            self._basis_key = key
        return self._basis

    def check_length(self, n):
        if ops.stft_frames(n, self.n_fft, self.hop_length) < 1:
            raise ValueError(f'MelSpectrogram: a clip of {n} samples is too short for the reflect padding of n_fft = {self.n_fft} '
                             f'(needs more than {self.n_fft // 2})')

    def _mel(self, x, x_from=None):
        """x fp32 [B, n] -> (mel [B, n_mels, T], the complex spectrum of the rows from x_from on or None, the basis)"""
        fb = self.mel_scale.fb
        if fb.device != x.device or fb.dtype != F32:
            raise RuntimeError(f'MelSpectrogram: buffers on {fb.device} ({fb.dtype}), input on {x.device}: move the module to the input\'s device in fp32')
        basis = self._dft_basis(x.device)
        left = (self.n_fft - self.win_length) // 2
        P, X = ops.mel_power(x, basis, self.n_fft, self.hop_length, left, left + self.win_length, x_from=x_from)
        return ops.mel_project(P, fb), X, basis

    def forward(self, x):
        """x fp32 (..., n) on the GPU -> (..., n_mels, T), T = n // hop_length + 1; differentiable in x"""
        self.check_length(x.shape[-1])
        lead = x.shape[:-1]
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        mel = _MelSpecFn.apply(x2, self) if _needs_graph(x2) else self._mel(x2.detach())[0]
        return mel.reshape(*lead, self.n_mels, mel.shape[-1])


def multi_spectral_recon_loss(orig, recon, transforms, alphas):
    """sum over scales of mean_{b,c,t} sum_m |Mo - Mr| + alpha mean_{b,c,t} ||log max(Mo, 1e-20) - log max(Mr, 1e-20)||_2 (soundstream.py:938-945),
    Mo / Mr the mel spectrograms of orig / recon (..., n).  The gradient goes to recon only; leading axes fold into the batch."""
    transforms, alphas = list(transforms), [float(a) for a in alphas]
    if len(transforms) != len(alphas):
        raise ValueError(f'multi_spectral_recon_loss: {len(transforms)} transforms but {len(alphas)} alphas')
    if orig.shape != recon.shape:
        raise ValueError(f'multi_spectral_recon_loss: orig {tuple(orig.shape)} and recon {tuple(recon.shape)} differ in shape')
    n = orig.shape[-1]
    for t in transforms:                                         # every refusal before any launch
        if not isinstance(t, MelSpectrogram):
            raise TypeError(f'multi_spectral_recon_loss takes audiolm_pytorch_amd.MelSpectrogram modules; got {type(t).__name__}')
        t.check_length(n)
    real, fake = _f32c(orig).detach().reshape(-1, n), _f32c(recon).reshape(-1, n)
    if not transforms:
        return torch.zeros((), dtype=F32, device=real.device)
    both = torch.cat((real, fake.detach()), dim=0)
    graph = _needs_graph(fake)
    total = None
    for t, alpha in zip(transforms, alphas):
        term = _MelLossFn.apply(fake, both, t, alpha) if graph else ops.mel_frame_loss(t._mel(both)[0], alpha)[0]
        total = term if total is None else total + term
    return total
