"""Wave discriminators of SoundStream training: the reference's `MultiScaleDiscriminator` (soundstream.py:92-140), the pooling between its
scales (:634) and the hinge / L1 / squared-error loss means (:61-65, :931, :976), on the fp32 kernels of csrc/discr.hip.

Parameter names and shapes are the reference's (`init_conv.*`, `conv_layers.{i}.0.*`, `final_conv.{0,2}.*`), so the `discriminators.*` entries of a
reference training checkpoint load.  The kernels read a conv weight in nn.Conv1d's own layout, so there is NO derived weight image to keep in step with
an optimizer: every launch takes the parameter's current storage.  A graph is built only with grad mode on and an input or parameter that requires
grad (train / eval mode makes no difference to these layers); otherwise a call issues the forward launches only.  Saved per conv: its input and, where
LeakyReLU follows, its output (the activation's derivative is taken from the output's sign).  Gradients are bitwise reproducible (no atomics).

`ComplexSTFTDiscriminator` (soundstream.py:173-310) follows the same rules on the kernels of csrc/stft_discr.hip: the STFT and every complex conv2d
are implicit GEMMs on the exact-fp32 matrix core, the parameters keep the reference's names and real-view storage (`init_conv.*`,
`layers.{i}.0.fn.{0,2}.*`, `layers.{i}.0.fn.1.b`, `layers.{i}.1.*`, `final_conv.*`), and `l1_loss` takes its complex64 intermediates.

Double backward (the gradient penalty, soundstream.py:70-83).  Every `backward` below issues its launches through an autograd Function of its own
(`_*BwdFn`, `_*DgradFn`), so that `torch.autograd.grad(..., create_graph=True)` records the input-gradient chain: a convolution is linear, so the
derivative of its input-gradient kernel with respect to the incoming gradient is its forward kernel and the one with respect to the weight is its
weight-gradient kernel, and the STFT likewise; ModReLU and |z| have second-order kernels.  Under a plain `backward()` torch runs these Functions without
recording: the same launches with the same arguments.  What is not twice differentiable (weight gradients, the pooling backward, the MSE / L1 backward)
raises `NotImplementedError` by name when something differentiates through it.  Nothing is differentiable a third time.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

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


_WAVE_GRAD_ONLY = [False]     # set by gradient_penalty around its first pass: only the wave's gradient is asked for there (needs_input_grad is fixed
                               # at forward time, so without it every weight gradient would be computed, recorded and thrown away)


def _params_wanted(*flags):
    return any(flags) and not _WAVE_GRAD_ONLY[0]


def _no_double_backward(what):
    raise NotImplementedError(f'double backward through {what} is not implemented (twice differentiable: the input gradients of the discriminator '
                              'convolutions, of the STFT, of ModReLU and of |z|, which is what the gradient penalty needs)')


class _GConvDgradFn(torch.autograd.Function):
    """dx = gconv1d_dgrad(g, y, w); d/dg = m(y) conv(v, w), d/dw = gconv1d_wgrad(g, y, v), d/dy = 0 almost everywhere"""

    @staticmethod
    def forward(ctx, g, y, weight, Cin, Tin, stride, padding, groups):
        ctx.cfg = (stride, padding, groups)
        ctx.save_for_backward(g, y, weight)
        return ops.gconv1d_dgrad(g, y, weight, Cin, Tin, stride=stride, padding=padding, groups=groups)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        g, y, weight = ctx.saved_tensors
        stride, padding, groups = ctx.cfg
        v = v.to(F32).contiguous()
        dg = dw = None
        if ctx.needs_input_grad[0]:
            dg = ops.gconv1d_fwd_masked(v, weight, y, stride=stride, padding=padding, groups=groups)
        if ctx.needs_input_grad[2]:
            dw = ops.gconv1d_wgrad(g, y, v, weight.shape[2], stride=stride, padding=padding, groups=groups)[0]
        return dg, None, dw, None, None, None, None, None


class _GConvWgradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, y, x, ksize, stride, padding, groups):
        return ops.gconv1d_wgrad(g, y, x, ksize, stride=stride, padding=padding, groups=groups)

    @staticmethod
    def backward(ctx, *_):
        _no_double_backward('the weight / bias gradient of a discriminator conv1d (gconv1d_wgrad)')


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
            dx = _GConvDgradFn.apply(g, y, weight, x.shape[1], x.shape[2], stride, padding, groups)
        if _params_wanted(ctx.needs_input_grad[1], ctx.needs_input_grad[2]):
            dw, db = _GConvWgradFn.apply(g, y, x, weight.shape[2], stride, padding, groups)
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


class _AvgPoolBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, T, f):
        return ops.avgpool1d_bwd(g, T, f)

    @staticmethod
    def backward(ctx, *_):
        _no_double_backward('the pooling backward (avgpool1d_bwd)')


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f):
        ctx.cfg = (x.shape[-1], f)
        return ops.avgpool1d(x, f)

    @staticmethod
    def backward(ctx, g):
        T, f = ctx.cfg
        return _AvgPoolBwdFn.apply(g.to(F32).contiguous(), T, f), None


class AvgPoolDownsample(nn.AvgPool1d):
    """nn.AvgPool1d(2 * factor, stride=factor, padding=factor) of the reference's `downsamples` (padding counts in the divisor), on the HIP kernel"""

    def __init__(self, factor):
        super().__init__(2 * factor, stride=factor, padding=factor)
        self.factor = factor

    def forward(self, x):
        x = _f32c(x)
        return _AvgPoolFn.apply(x, self.factor) if _needs_graph(x) else ops.avgpool1d(x, self.factor)


_LOSS_NAMES = {ops.LOSS_L1: 'the L1 loss', ops.LOSS_MSE: 'the squared-error loss', ops.LOSS_L1_COMPLEX: 'the complex L1 loss'}


class _LossBwdFn(torch.autograd.Function):
    """the backward of a loss mean whose derivative depends on its operands (L1, squared error, complex L1): not twice differentiable, by name"""

    @staticmethod
    def forward(ctx, a, b, g, mode, need_a, need_b):
        ctx.mode = mode
        return ops.loss_mean_bwd(mode, a, b, g, need_a, need_b)

    @staticmethod
    def backward(ctx, *_):
        _no_double_backward(f'the backward of {_LOSS_NAMES[ctx.mode]} (loss_mean_bwd)')


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
        g = g.to(F32).contiguous()
        if ctx.mode in (ops.LOSS_HINGE_DISCR, ops.LOSS_HINGE_GEN):
            # piecewise constant in the operands: the result is a constant of a second pass, which is its exact derivative almost everywhere
            da, db = ops.loss_mean_bwd(ctx.mode, a.detach(), None if b is None else b.detach(), g.detach(), ctx.needs_input_grad[0], need_b)
        else:
            da, db = _LossBwdFn.apply(a, b, g, ctx.mode, ctx.needs_input_grad[0], need_b)
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
    """F.l1_loss; on a pair of complex64 tensors the mean modulus |a - b| over complex elements"""
    if a.is_complex() or b.is_complex():
        if a.dtype != torch.complex64 or b.dtype != torch.complex64:
            raise TypeError(f'l1_loss: a complex pair must be complex64 on both sides; got {a.dtype} and {b.dtype}')
        return _loss(ops.LOSS_L1_COMPLEX, torch.view_as_real(a), torch.view_as_real(b))
    return _loss(ops.LOSS_L1, a, b)


def mse_loss(a, b):
    return _loss(ops.LOSS_MSE, a, b)


class _GradPenaltyFn(torch.autograd.Function):
    """weight * mean_r (|G_r| - center)^2 of G [R, n] (csrc/discr.hip); its backward is a plain kernel"""

    @staticmethod
    def forward(ctx, G, weight, center):
        out, norms = ops.grad_penalty(G, weight, center)
        ctx.cfg = (weight, center)
        ctx.save_for_backward(G, norms)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        G, norms = ctx.saved_tensors
        return ops.grad_penalty_bwd(G, norms, gout.to(F32).contiguous(), *ctx.cfg), None, None


def penalty_of_gradients(gradients, weight=10, center=0.):
    """weight * mean_b (|G_b|_2 - center)^2 of the gradients (b, ...), the norm per batch row over everything else: the reduction of
    `gradient_penalty`, differentiable once with respect to the gradients"""
    G = _f32c(gradients).reshape(gradients.shape[0], -1)
    return _GradPenaltyFn.apply(G, float(weight), float(center)) if _needs_graph(G) else ops.grad_penalty(G, float(weight), float(center))[0]


def wave_gradients(wave, output):
    """d output / d wave with `create_graph=True` (grad_outputs: ones), the first pass of `gradient_penalty`.  Only the wave's gradient is taken:
    the native backward passes skip their parameter gradients meanwhile."""
    _WAVE_GRAD_ONLY[0] = True
    try:
        return torch.autograd.grad(outputs=output, inputs=wave, grad_outputs=torch.ones_like(output), create_graph=True, retain_graph=True,
                                   only_inputs=True)[0]
    finally:
        _WAVE_GRAD_ONLY[0] = False


def gradient_penalty(wave, output, weight=10, center=0.):       # soundstream.py:70-83
    """weight * mean_b (|d output / d wave_b|_2 - center)^2; the result backpropagates into whatever `output` depends on (double backward)"""
    return penalty_of_gradients(wave_gradients(wave, output), weight, center)


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


# ---- ComplexSTFTDiscriminator (soundstream.py:173-310) on the kernels of csrc/stft_discr.hip.  Inside the module a complex activation travels as its
# fp32 [..., 2] (re, im) view; the intermediates handed out are torch.complex64 views of the same storage (view_as_complex: no copy, no kernel).

class _StftBwdFn(torch.autograd.Function):
    """dx = stft_bwd(g); d/dg = stft(v)"""

    @staticmethod
    def forward(ctx, g, basis, n, n_fft, hop):
        ctx.cfg = (n_fft, hop)
        ctx.basis = basis
        return ops.stft_bwd(g, basis, n, n_fft, hop)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        n_fft, hop = ctx.cfg
        return ops.stft(v.to(F32).contiguous(), ctx.basis, n_fft, hop), None, None, None, None


class _StftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, basis, n_fft, hop):
        ctx.cfg = (x.shape[1], n_fft, hop)
        ctx.basis = basis
        return ops.stft(x, basis, n_fft, hop)

    @staticmethod
    def backward(ctx, g):
        n, n_fft, hop = ctx.cfg
        return _StftBwdFn.apply(g.to(F32).contiguous(), ctx.basis, n, n_fft, hop), None, None, None


class _CConvDgradFn(torch.autograd.Function):
    """dx = cconv2d_dgrad(g, w); d/dg = cconv2d(v, w) without bias or residual, d/dw = cconv2d_wgrad(g, v)"""

    @staticmethod
    def forward(ctx, g, weight, H, W, stride, padding):
        ctx.cfg = (stride, padding)
        ctx.save_for_backward(g, weight)
        return ops.cconv2d_dgrad(g, weight, H, W, stride=stride, padding=padding)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        g, weight = ctx.saved_tensors
        stride, padding = ctx.cfg
        v = v.to(F32).contiguous()
        dg = dw = None
        if ctx.needs_input_grad[0]:
            dg = ops.cconv2d(v, weight, None, stride=stride, padding=padding)
        if ctx.needs_input_grad[1]:
            dw = ops.cconv2d_wgrad(g, v, weight.shape[2:4], stride=stride, padding=padding)[0]
        return dg, dw, None, None, None, None


class _CConvWgradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, kernel_size, stride, padding):
        return ops.cconv2d_wgrad(g, x, kernel_size, stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, *_):
        _no_double_backward('the weight / bias gradient of a complex conv2d (cconv2d_wgrad)')


class _CConv2dFn(torch.autograd.Function):
    """conv2d of (re, im) pairs + bias (+ residual)"""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, padding):
        ctx.cfg = (stride, padding)
        ctx.save_for_backward(x, weight)
        return ops.cconv2d(x, weight.detach(), bias.detach(), stride=stride, padding=padding, residual=residual)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        stride, padding = ctx.cfg
        g = g.to(F32).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _CConvDgradFn.apply(g, weight, x.shape[2], x.shape[3], stride, padding)
        if _params_wanted(ctx.needs_input_grad[1], ctx.needs_input_grad[2]):
            dw, db = _CConvWgradFn.apply(g, x, tuple(weight.shape[2:4]), stride, padding)
        return dx, dw, db, (g if ctx.needs_input_grad[3] else None), None, None


class _ModReLUBwdFn(torch.autograd.Function):
    """(dz, db) = modrelu_bwd(g, z, b); its derivatives against the cotangents (v, beta) in one launch (csrc/stft_discr.hip modrelu_bwd2_kernel)"""

    @staticmethod
    def forward(ctx, g, z, b, need_dz):
        ctx.save_for_backward(g, z, b)
        ctx.need_dz = need_dz
        dz, db = ops.modrelu_bwd(g, z, b, need_dz=need_dz)
        return dz, db

    @staticmethod
    @once_differentiable
    def backward(ctx, v, beta):
        g, z, b = ctx.saved_tensors
        v = v.to(F32).contiguous() if ctx.need_dz else None
        dg, dz, db = ops.modrelu_bwd2(g, z, b, v, beta.to(F32).contiguous(), need_dz=ctx.needs_input_grad[1])
        return dg, dz, (db if ctx.needs_input_grad[2] else None), None


class _ModReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, b):
        ctx.save_for_backward(z, b)
        return ops.modrelu(z, b.detach())

    @staticmethod
    def backward(ctx, g):
        z, b = ctx.saved_tensors
        dz, db = _ModReLUBwdFn.apply(g.to(F32).contiguous(), z, b, ctx.needs_input_grad[0])
        return dz, (db if ctx.needs_input_grad[1] else None)


class _CAbsBwdFn(torch.autograd.Function):
    """dz = complex_abs_bwd(g, z) = g u; d/dg = u . v, d/dz = g P v / |z|"""

    @staticmethod
    def forward(ctx, g, z):
        ctx.save_for_backward(g, z)
        return ops.complex_abs_bwd(g, z)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        g, z = ctx.saved_tensors
        dg, dz = ops.complex_abs_bwd2(g, z, v.to(F32).contiguous(), need_dz=ctx.needs_input_grad[1])
        return dg, dz


class _CAbsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return ops.complex_abs(z)

    @staticmethod
    def backward(ctx, g):
        z, = ctx.saved_tensors
        return _CAbsBwdFn.apply(g.to(F32).contiguous(), z)


def _as_pairs(x):
    """a complex64 tensor or its fp32 [..., 2] view -> the contiguous fp32 [..., 2] view"""
    if x.is_complex():
        if x.dtype != torch.complex64:
            raise TypeError(f'the discriminator kernels are fp32 (complex64); got {x.dtype}')
        x = torch.view_as_real(x)
    return _f32c(x)


class ModReLU(nn.Module):                                        # soundstream.py:173-183
    def __init__(self):
        super().__init__()
        self.b = nn.Parameter(torch.tensor(0.))

    def forward(self, z):
        """z complex64 or fp32 [..., 2] -> fp32 [..., 2]; the scalar b is read on the device"""
        z, b = _as_pairs(z), _f32c(self.b)
        return _ModReLUFn.apply(z, b) if _needs_graph(z, self.b) else ops.modrelu(z.detach(), b.detach())


class ComplexConv2d(nn.Module):                                  # soundstream.py:185-206
    """weight [Cout, Cin, kh, kw, 2] and bias [Cout, 2] are view_as_real of a complex64 nn.Conv2d's parameters, initialised by that module on the CPU
    like the reference does (the same torch.manual_seed gives the same values); the kernels read them as they are."""

    def __init__(self, dim, dim_out, kernel_size, stride=1, padding=0):
        super().__init__()
        conv = nn.Conv2d(dim, dim_out, kernel_size, dtype=torch.complex64)
        self.weight = nn.Parameter(torch.view_as_real(conv.weight))
        self.bias = nn.Parameter(torch.view_as_real(conv.bias))
        self.stride = stride
        self.padding = padding

    def forward(self, x, residual=None):
        """x complex64 or fp32 [b, c, h, w, 2] -> fp32 [b, c', h', w', 2] (+ residual)"""
        x, w, b = _as_pairs(x), _f32c(self.weight), _f32c(self.bias)
        if _needs_graph(x, self.weight, self.bias, residual):
            return _CConv2dFn.apply(x, w, b, residual, self.stride, self.padding)
        return ops.cconv2d(x.detach(), w.detach(), b.detach(), stride=self.stride, padding=self.padding,
                           residual=None if residual is None else residual.detach())


class _ComplexResidual(nn.Module):                               # soundstream.py:314-320 around Sequential(conv, ModReLU, conv)
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        x = _as_pairs(x)
        return self.fn[2](self.fn[1](self.fn[0](x)), residual=x)     # the residual add is the second conv's epilogue


def _complex_stft_residual_unit(chan_in, chan_out, strides):     # soundstream.py:208-219
    kernel_sizes = tuple(s + 2 for s in strides)
    paddings = tuple(k // 2 for k in kernel_sizes)
    return nn.Sequential(
        _ComplexResidual(nn.Sequential(ComplexConv2d(chan_in, chan_in, 3, padding=1), ModReLU(), ComplexConv2d(chan_in, chan_in, 3, padding=1))),
        ComplexConv2d(chan_in, chan_out, kernel_sizes, stride=strides, padding=paddings))


class ComplexSTFTDiscriminator(nn.Module):                       # soundstream.py:221-310
    def __init__(self, *, channels=32, strides=((1, 2), (2, 2), (1, 2), (2, 2), (1, 2), (2, 2)), chan_mults=(1, 2, 4, 4, 8, 8), input_channels=1,
                 n_fft=1024, hop_length=256, win_length=1024, stft_normalized=False, stft_window_fn=torch.hann_window, logits_abs=True):
        super().__init__()
        self.input_channels = input_channels
        self.init_conv = ComplexConv2d(input_channels, channels, 7, padding=3)
        layer_channels = (channels, *(m * channels for m in chan_mults))
        self.layers = nn.ModuleList([_complex_stft_residual_unit(ci, co, tuple(s))
                                     for s, (ci, co) in zip(strides, zip(layer_channels[:-1], layer_channels[1:]))])
        self.final_conv = ComplexConv2d(layer_channels[-1], 1, (16, 1))
        self.stft_normalized = stft_normalized
        self.stft_window_fn = stft_window_fn
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.logits_abs = logits_abs

    def _convs(self):
        yield self.init_conv
        for layer in self.layers:
            yield from (layer[0].fn[0], layer[0].fn[2], layer[1])
        yield self.final_conv

    def check_geometry(self, n):
        """the refusals that need no launch: the clip against the reflect padding, and every conv's input against its kernel (the frequency axis
        against the final conv's 16 rows)"""
        if self.input_channels != 1:
            raise NotImplementedError("ComplexSTFTDiscriminator: input_channels != 1 (the reference's own rearrange 'b 1 n -> b n' does not admit it)")
        T = ops.stft_frames(n, self.n_fft, self.hop_length)
        if T < 1:
            raise ValueError(f'ComplexSTFTDiscriminator: a clip of {n} samples is too short for the reflect padding of n_fft = {self.n_fft} '
                             f'(needs more than {self.n_fft // 2})')
        hw = (self.n_fft // 2 + 1, T)
        for conv in self._convs():
            out = ops.cconv2d_out_hw(*hw, tuple(conv.weight.shape[2:4]), conv.stride, conv.padding)
            if out is None:
                raise ValueError(f'ComplexSTFTDiscriminator: the frequency axis shrinks to {hw[0]} rows, fewer than the '
                                 f'{conv.weight.shape[2]} rows of the final conv (n_fft = {self.n_fft} is too small for these strides)')
            hw = out
        return hw

    def forward(self, x, return_intermediates=False):
        """x fp32 (b, 1, n) -> logits: real (b, 1, f', t') with logits_abs, else the trailing-2 real view (b, 1, f', t', 2); with
        return_intermediates also the complex64 outputs of init_conv and of every layer"""
        self.check_geometry(x.shape[-1])
        if x.ndim != 3 or x.shape[1] != 1:
            raise ValueError(f'ComplexSTFTDiscriminator takes a wave of shape (b, 1, n); got {tuple(x.shape)}')
        x = _f32c(x).reshape(x.shape[0], x.shape[-1])
        window = self.stft_window_fn(self.win_length, device='cpu')
        basis = ops.stft_basis(self.n_fft, window, self.stft_normalized, x.device)
        if _needs_graph(x):                                          # the STFT has no parameters: its backward runs only for the wave
            h = _StftFn.apply(x, basis, self.n_fft, self.hop_length)
        else:
            h = ops.stft(x.detach(), basis, self.n_fft, self.hop_length)
        h = self.init_conv(h.unsqueeze(1))
        intermediates = [h]
        for layer in self.layers:
            h = layer[1](layer[0](h))
            intermediates.append(h)
        z = self.final_conv(h)
        if self.logits_abs:
            logits = _CAbsFn.apply(z) if _needs_graph(z) else ops.complex_abs(z)
        else:
            logits = z
        if not return_intermediates:
            return logits
        return logits, [torch.view_as_complex(t) for t in intermediates]
