"""Plain-torch restatement of the reference's ComplexSTFTDiscriminator (soundstream.py:173-310), written for this project: torch.stft, complex
F.conv2d and the ModReLU formula.  Runs in float64 or fp32 on the CPU (or anywhere PyTorch runs a complex conv) and is the reference of the
module-level tests; `probe` collects the ModReLU pre-activations |z| + b and the complex logits for the margin checks."""
import torch
import torch.nn.functional as F
from torch import nn


def _complex_dtype(real_dtype):
    return torch.complex128 if real_dtype == torch.float64 else torch.complex64


class ModReLURestated(nn.Module):
    def __init__(self):
        super().__init__()
        self.b = nn.Parameter(torch.tensor(0.))
        self.probe = None

    def forward(self, z):
        pre = torch.abs(z) + self.b
        if self.probe is not None:
            self.probe.append(pre.detach().reshape(-1))
        return F.relu(pre) * torch.exp(1.j * torch.angle(z))


class ComplexConv2dRestated(nn.Module):
    def __init__(self, dim, dim_out, kernel_size, stride=1, padding=0):
        super().__init__()
        conv = nn.Conv2d(dim, dim_out, kernel_size, dtype=torch.complex64)
        self.weight = nn.Parameter(torch.view_as_real(conv.weight))
        self.bias = nn.Parameter(torch.view_as_real(conv.bias))
        self.stride, self.padding = stride, padding

    def forward(self, x):
        weight, bias = torch.view_as_complex(self.weight), torch.view_as_complex(self.bias)
        return F.conv2d(x.to(weight.dtype), weight, bias, stride=self.stride, padding=self.padding)


class ResidualRestated(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x) + x


def residual_unit(chan_in, chan_out, strides):
    kernel_sizes = tuple(s + 2 for s in strides)
    paddings = tuple(k // 2 for k in kernel_sizes)
    return nn.Sequential(
        ResidualRestated(nn.Sequential(ComplexConv2dRestated(chan_in, chan_in, 3, padding=1), ModReLURestated(),
                                       ComplexConv2dRestated(chan_in, chan_in, 3, padding=1))),
        ComplexConv2dRestated(chan_in, chan_out, kernel_sizes, stride=strides, padding=paddings))


class ComplexSTFTDiscriminatorRestated(nn.Module):
    def __init__(self, *, channels=32, strides=((1, 2), (2, 2), (1, 2), (2, 2), (1, 2), (2, 2)), chan_mults=(1, 2, 4, 4, 8, 8), input_channels=1,
                 n_fft=1024, hop_length=256, win_length=1024, stft_normalized=False, stft_window_fn=torch.hann_window, logits_abs=True):
        super().__init__()
        self.init_conv = ComplexConv2dRestated(input_channels, channels, 7, padding=3)
        chans = (channels, *(m * channels for m in chan_mults))
        self.layers = nn.ModuleList([residual_unit(ci, co, tuple(s)) for s, (ci, co) in zip(strides, zip(chans[:-1], chans[1:]))])
        self.final_conv = ComplexConv2dRestated(chans[-1], 1, (16, 1))
        self.stft_normalized, self.stft_window_fn = stft_normalized, stft_window_fn
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.logits_abs = logits_abs
        self.complex_logits = None

    def probe(self, on=True):
        """start (or stop) collecting the ModReLU pre-activations; returns the lists' owner for reading"""
        for m in self.modules():
            if isinstance(m, ModReLURestated):
                m.probe = [] if on else None
        return self

    def pre_activations(self):
        return torch.cat([torch.cat(m.probe) for m in self.modules() if isinstance(m, ModReLURestated) and m.probe])

    def forward(self, x, return_intermediates=False):
        assert x.ndim == 3 and x.shape[1] == 1
        x = x[:, 0]
        window = self.stft_window_fn(self.win_length, device=x.device).to(x.dtype)
        x = torch.stft(x, self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=window, normalized=self.stft_normalized,
                       return_complex=True)
        x = self.init_conv(x[:, None])
        intermediates = [x]
        for layer in self.layers:
            x = layer(x)
            intermediates.append(x)
        z = self.final_conv(x)
        self.complex_logits = z.detach()
        logits = z.abs() if self.logits_abs else torch.view_as_real(z)
        if not return_intermediates:
            return logits
        return logits, intermediates
