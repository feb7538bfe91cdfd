"""GPU windowed-sinc resampling: `resample(waveform, orig_freq, new_freq, ...)` with torchaudio.functional.resample's signature and results.

The reference codec resamples its input to the codec rate whenever a rate is given (soundstream.py:779-795: process_input calls
torchaudio.functional.resample).  torchaudio is not part of this stack, so its polyphase recipe (third-party, published) is restated here:
  g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * rolloff, W = ceil(lw * o / base), T = 2 W + o taps;
  table K[p, k] (p < n, k < T) in fp32, in torchaudio's operation order:
    t = (-p / n + (k - W) / o) * base, clamped to [-lw, lw];  window w = cos(t pi / lw / 2)^2 (hann) or i0(beta sqrt(1 - (t / lw)^2)) / i0(beta)
    (kaiser);  t *= pi;  K = (t == 0 ? 1 : sin(t) / t) * (w * base / o)
  rows of L samples, zero-padded by W on the left and W + o on the right:  y[j n + p] = sum_k K[p, k] xpad[j o + k], truncated to ceil(n L / o).
The table is built once per (device, o, n, method, lw, rolloff, beta) on the host with torch CPU ops and uploaded; the correlation (and its
adjoint, for autograd) runs in csrc/resample.hip.  There is no CPU path: a CPU tensor raises AlmError unless orig == new.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from . import _lib, ops

F32 = torch.float32
KAISER_BETA = 14.769656459379492          # torchaudio's default beta for sinc_interp_kaiser
_METHODS = ('sinc_interp_hann', 'sinc_interp_kaiser')
_CACHE_MAX = 32
_cache: 'OrderedDict[tuple, torch.Tensor]' = OrderedDict()


def _rates(orig_freq, new_freq):
    for f in (orig_freq, new_freq):
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not math.isfinite(f) or int(f) != f:
            raise ValueError(f'sample rates must be integer-valued, got {orig_freq} and {new_freq}')
        if f <= 0:
            raise ValueError(f'sample rates must be positive, got {orig_freq} and {new_freq}')
    return int(orig_freq), int(new_freq)


def geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> (o, n, W, T): the rates over their gcd, the filter half-width W in input samples and the taps per phase T = 2 W + o."""
    orig, new = _rates(orig_freq, new_freq)
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    W = math.ceil(lowpass_filter_width * o / base)
    return o, n, W, 2 * W + o


def output_length(length, orig_freq, new_freq):
    """ceil(new * length / orig) with the rates over their gcd (exact integer arithmetic)"""
    o, n, _, _ = geometry(orig_freq, new_freq)
    return (n * length + o - 1) // o


def sinc_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann', beta=None):
    """the polyphase table K fp32 [n, T] on the CPU, built in torchaudio's operation order (its rounding is visible at the 1e-5 level)"""
    if resampling_method not in _METHODS:
        raise ValueError(f'Invalid resampling method: {resampling_method}')
    if lowpass_filter_width <= 0:
        raise ValueError('Low pass filter width should be positive.')
    o, n, W, _ = geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    base = min(o, n) * rolloff
    idx = torch.arange(-W, W + o, dtype=F32)[None] / o
    t = torch.arange(0, -n, -1, dtype=F32)[:, None] / n + idx
    t *= base
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    if resampling_method == 'sinc_interp_hann':
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    else:
        beta_t = torch.tensor(float(KAISER_BETA if beta is None else beta))
        window = torch.i0(beta_t * torch.sqrt(1 - (t / lowpass_filter_width) ** 2)) / torch.i0(beta_t)
    t *= math.pi
    scale = base / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels


def _device_table(device, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta):
    o, n, _, _ = geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    key = (device, o, n, resampling_method, float(lowpass_filter_width), float(rolloff),
           None if resampling_method == 'sinc_interp_hann' else float(KAISER_BETA if beta is None else beta))
    tab = _cache.get(key)
    if tab is None:
        tab = sinc_table(o, n, lowpass_filter_width, rolloff, resampling_method, beta).to(device)
        _cache[key] = tab
        while len(_cache) > _CACHE_MAX:
            _cache.popitem(last=False)
    else:
        _cache.move_to_end(key)
    return tab


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, o, n, W):
        ctx.geom = (x.shape[-1], o, n, W)
        ctx.save_for_backward(table)
        return ops.resample_sinc(x, table, o, n, W)

    @staticmethod
    def backward(ctx, dy):
        L, o, n, W = ctx.geom
        table, = ctx.saved_tensors
        return ops.resample_sinc_bwd(dy.to(F32), table, L, o, n, W), None, None, None, None


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann', beta=None):
    """torchaudio.functional.resample on the MI355X: resamples the last dimension of `waveform` from `orig_freq` to `new_freq` Hz with a
    windowed-sinc polyphase filter (hann or kaiser window), the same results as torchaudio's fp32 path up to fp32 summation order.

    The arithmetic is fp32 for every float dtype (torchaudio builds its filter in the input dtype): a bf16 / fp16 input is widened, resampled
    and the result comes back in the input's dtype.  Differentiable (the backward is the adjoint kernel).  orig_freq == new_freq returns
    `waveform` itself.  TypeError for a non-float tensor, ValueError for rates that are not positive integers, an unknown method or a
    non-positive filter width, AlmError for a CPU tensor (there is no CPU path)."""
    if not torch.is_tensor(waveform) or not waveform.is_floating_point():
        raise TypeError(f'Expected floating point type for waveform tensor, but received {getattr(waveform, "dtype", type(waveform))}.')
    orig, new = _rates(orig_freq, new_freq)
    if resampling_method not in _METHODS:
        raise ValueError(f'Invalid resampling method: {resampling_method}')
    if lowpass_filter_width <= 0:
        raise ValueError('Low pass filter width should be positive.')
    if orig == new:
        return waveform
    if waveform.dim() == 0:
        raise ValueError('waveform needs a time dimension')
    if not waveform.is_cuda:
        raise _lib.AlmError('audiolm_pytorch_amd.resample runs on the MI355X only (got a CPU tensor); there is no CPU fallback')
    o, n, W, _ = geometry(orig, new, lowpass_filter_width, rolloff)
    table = _device_table(waveform.device, orig, new, lowpass_filter_width, rolloff, resampling_method, beta)
    lead, L = waveform.shape[:-1], waveform.shape[-1]
    x = waveform.reshape(math.prod(lead), L)
    y = _Resample.apply(x if x.dtype == F32 else x.to(F32), table, o, n, W)
    return y.reshape(*lead, y.shape[-1]).to(waveform.dtype)
