"""Wave discriminators of SoundStream training: the reference's `MultiScaleDiscriminator` (soundstream.py:92-140), the pooling between its
scales (:634) and the hinge / L1 / squared-error loss means (:61-65, :931, :976), on the fp32 kernels of csrc/discr.hip.

Parameter names and shapes are the reference's (`init_conv.*`, `conv_layers.{i}.0.*`, `final_conv.{0,2}.*`), so the `discriminators.*` entries of a
reference training checkpoint load.  The kernels read a conv weight in nn.Conv1d's own layout, so there is NO derived weight image to keep in step with
an optimizer: every launch takes the parameter's current storage.  A graph is built only with grad mode on and an input or parameter that requires
grad (train / eval mode makes no difference to these layers); otherwise a call issues the forward launches only.  Saved per conv: its input and, where
LeakyReLU follows, its output (the activation's derivative is taken from the output's sign).  Gradients are bitwise reproducible (no atomics).
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops

F32 = torch.float32


def _needs_graph(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _f32c(t):
    if not t.is_cuda:
        raise RuntimeError('audiolm_pytorch_amd discriminators run on the MI355X only (no CPU fallback)')
    if t.dtype != F32:
        raise TypeError(f'the discriminator kernels are fp32; got {t.dtype}')
    return t.contiguous()


class _GConv1dFn(torch.autograd.Function):
    """act(conv1d(x, w, b, stride, padding, groups)), act = LeakyReLU(0.1) or identity"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, groups, leaky):
        y = ops.gconv1d(x, weight.detach(), bias.detach(), stride=stride, padding=padding, groups=groups, leaky=leaky)
        ctx.cfg = (stride, padding, groups)
        ctx.save_for_backward(x, weight, y if leaky else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        stride, padding, groups = ctx.cfg
        g = g.to(F32).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.gconv1d_dgrad(g, y, weight.detach(), x.shape[1], x.shape[2], stride=stride, padding=padding, groups=groups)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = ops.gconv1d_wgrad(g, y, x, weight.shape[2], stride=stride, padding=padding, groups=groups)
        return dx, dw, db, None, None, None, None


def conv1d_act(conv: nn.Conv1d, x, leaky=False):
    """an nn.Conv1d (zero padding, dilation 1) followed by LeakyReLU(0.1) or nothing, on the HIP kernels"""
    if conv.dilation != (1,) or conv.padding_mode != 'zeros' or isinstance(conv.padding, str) or conv.bias is None:
        raise NotImplementedError('the discriminator conv kernels cover zero-padded, undilated nn.Conv1d with a bias')
    x, w, b = _f32c(x), _f32c(conv.weight), _f32c(conv.bias)
    stride, padding, groups = conv.stride[0], conv.padding[0], conv.groups
    if _needs_graph(x, conv.weight, conv.bias):
        return _GConv1dFn.apply(x, w, b, stride, padding, groups, leaky)
    return ops.gconv1d(x.detach(), w.detach(), b.detach(), stride=stride, padding=padding, groups=groups, leaky=leaky)


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f):
        ctx.cfg = (x.shape[-1], f)
        return ops.avgpool1d(x, f)

    @staticmethod
    def backward(ctx, g):
        T, f = ctx.cfg
        return ops.avgpool1d_bwd(g.to(F32).contiguous(), T, f), None


class AvgPoolDownsample(nn.AvgPool1d):
    """nn.AvgPool1d(2 * factor, stride=factor, padding=factor) of the reference's `downsamples` (padding counts in the divisor), on the HIP kernel"""

    def __init__(self, factor):
        super().__init__(2 * factor, stride=factor, padding=factor)
        self.factor = factor

    def forward(self, x):
        x = _f32c(x)
        return _AvgPoolFn.apply(x, self.factor) if _needs_graph(x) else ops.avgpool1d(x, self.factor)


class _LossMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mode):
        ctx.mode = mode
        ctx.save_for_backward(a, b)
        return ops.loss_mean(mode, a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        need_b = b is not None and ctx.needs_input_grad[1]
        da, db = ops.loss_mean_bwd(ctx.mode, a, b, g.to(F32).contiguous(), ctx.needs_input_grad[0], need_b)
        return da, db, None


def _loss(mode, a, b=None):
    a = _f32c(a)
    b = None if b is None else _f32c(b)
    if b is not None and b.shape != a.shape:
        raise ValueError(f'loss operands differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}')
    if _needs_graph(a, b):
        return _LossMeanFn.apply(a, b, mode)
    return ops.loss_mean(mode, a, b)


def hinge_discr_loss(fake, real):                                # soundstream.py:61-62
    return _loss(ops.LOSS_HINGE_DISCR, fake, real)


def hinge_gen_loss(fake):                                        # soundstream.py:64-65
    return _loss(ops.LOSS_HINGE_GEN, fake)


def l1_loss(a, b):
    return _loss(ops.LOSS_L1, a, b)


def mse_loss(a, b):
    return _loss(ops.LOSS_MSE, a, b)


class MultiScaleDiscriminator(nn.Module):                        # soundstream.py:92-140
    def __init__(self, channels=16, layers=4, groups=(4, 16, 64, 256), chan_max=1024, input_channels=1):
        super().__init__()
        self.init_conv = nn.Conv1d(input_channels, channels, 15, padding=7)
        self.conv_layers = nn.ModuleList([])
        curr = channels
        for _, group in zip(range(layers), groups):
            chan_out = min(curr * 4, chan_max)
            self.conv_layers.append(nn.Sequential(nn.Conv1d(curr, chan_out, 41, stride=4, padding=20, groups=group), nn.LeakyReLU(0.1)))
            curr = chan_out
        self.final_conv = nn.Sequential(nn.Conv1d(curr, curr, 5, padding=2), nn.LeakyReLU(0.1), nn.Conv1d(curr, 1, 3, padding=1))

    def forward(self, x, return_intermediates=False):
        """x fp32 (b, input_channels, n) -> logits (b, 1, n'), with return_intermediates also the outputs of the `conv_layers`"""
        x = conv1d_act(self.init_conv, x)
        intermediates = []
        for layer in self.conv_layers:
            x = conv1d_act(layer[0], x, leaky=True)
            intermediates.append(x)
        out = conv1d_act(self.final_conv[2], conv1d_act(self.final_conv[0], x, leaky=True))
        if not return_intermediates:
            return out
        return out, intermediates
