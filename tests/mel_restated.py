"""Test oracle: `torchaudio.transforms.MelSpectrogram` and the multi-spectral reconstruction loss of the reference, in plain PyTorch.

RESTATED from torchaudio's published implementation (torchaudio/transforms/_transforms.py: MelSpectrogram = Spectrogram + MelScale;
torchaudio/functional/functional.py: spectrogram, melscale_fbanks), for the subset of the signature the reference's SoundStream uses
(soundstream.py:662-669): sample_rate, n_fft, win_length, hop_length, n_mels, normalized; everything else at torchaudio's defaults (f_min = 0,
f_max = sample_rate / 2, power = 2, periodic Hann window, center = True, pad_mode = 'reflect', onesided, norm = None, mel_scale = 'htk').
torchaudio is not installed on this project's machines and cannot be: NOBODY has been able to compare this restatement against an installed torchaudio
here.  What it pins is the definition written down in this file; the native module (audiolm_pytorch_amd/mel_loss.py) is tested against it.

Dtype-generic (`.double()` gives the float64 reference; torchaudio itself builds window and filterbank in float32), with torchaudio's two persistent
buffers under torchaudio's names: `spectrogram.window` (win_length,) and `mel_scale.fb` (n_fft // 2 + 1, n_mels).

`multi_spectral_recon_loss_restated` is reference soundstream.py:938-945 line for line."""
import math

import torch
from torch import nn
from torch.linalg import vector_norm


def melscale_fbanks_restated(n_freqs, f_min, f_max, n_mels, sample_rate, dtype=torch.float64):
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_min = 2595.0 * math.log10(1.0 + (f_min / 700.0))
    m_max = 2595.0 * math.log10(1.0 + (f_max / 700.0))
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down_slopes = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up_slopes = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(down_slopes, up_slopes))


class _Spectrogram(nn.Module):
    def __init__(self, n_fft, win_length, hop_length, normalized):
        super().__init__()
        self.n_fft, self.win_length, self.hop_length, self.normalized = n_fft, win_length, hop_length, normalized
        self.register_buffer('window', torch.hann_window(win_length, dtype=torch.float64))

    def forward(self, x):
        shape = x.shape
        spec = torch.stft(x.reshape(-1, shape[-1]), self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=self.window, center=True,
                          pad_mode='reflect', normalized=False, onesided=True, return_complex=True)
        spec = spec.reshape(shape[:-1] + spec.shape[-2:])
        if self.normalized:                                      # torchaudio's normalized=True is "window": 1 / sqrt(sum w^2), not torch.stft's 1 / sqrt(n_fft)
            spec = spec / self.window.pow(2.).sum().sqrt()
        return spec.abs().pow(2.)


class _MelScale(nn.Module):
    def __init__(self, n_mels, sample_rate, n_stft):
        super().__init__()
        self.register_buffer('fb', melscale_fbanks_restated(n_stft, 0., float(sample_rate // 2), n_mels, sample_rate))

    def forward(self, spec):
        return torch.matmul(spec.transpose(-1, -2), self.fb).transpose(-1, -2)


class MelSpectrogramRestated(nn.Module):
    """buffers are built in float64; `.float()` / `.double()` choose the precision of the evaluation"""

    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, n_mels=128, normalized=False):
        super().__init__()
        win_length = win_length if win_length is not None else n_fft
        hop_length = hop_length if hop_length is not None else win_length // 2
        self.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels, self.normalized = sample_rate, n_fft, win_length, hop_length, n_mels, normalized
        self.spectrogram = _Spectrogram(n_fft, win_length, hop_length, normalized)
        self.mel_scale = _MelScale(n_mels, sample_rate, n_fft // 2 + 1)

    def forward(self, waveform):
        return self.mel_scale(self.spectrogram(waveform))


def log(t, eps=1e-20):
    return torch.log(t.clamp(min=eps))


def multi_spectral_recon_loss_restated(orig_x, recon_x, mel_spec_transforms, mel_spec_recon_alphas):
    multi_spectral_recon_loss = 0.
    for mel_transform, alpha in zip(mel_spec_transforms, mel_spec_recon_alphas):
        orig_mel, recon_mel = map(mel_transform, (orig_x, recon_x))
        log_orig_mel, log_recon_mel = map(log, (orig_mel, recon_mel))

        l1_mel_loss = (orig_mel - recon_mel).abs().sum(dim=-2).mean()
        l2_log_mel_loss = alpha * vector_norm(log_orig_mel - log_recon_mel, dim=-2).mean()

        multi_spectral_recon_loss = multi_spectral_recon_loss + l1_mel_loss + l2_log_mel_loss
    return multi_spectral_recon_loss
