"""Autograd layer of the codec's conv stacks: `torch.autograd.Function`s over the backward kernels of csrc/codec_bwd.hip for CausalConv1d,
CausalConvTranspose1d and the ResidualUnit (reference soundstream.py:332-369), plus the layout transpose.  soundstream.py takes them ONLY in training
mode with grad mode on and an input or parameter that requires grad; every other call issues the forward launches it always did.

The forward of each Function runs the SAME forward kernels as the eval path (the ResidualUnit as its two alm_conv1d_causal launches, to which the
fused alm_resunit_causal is bitwise equal, with the skip added by alm_add_f32), so a training-mode output is bitwise the eval-mode output.
Saved per ResidualUnit: its input x, the intermediate h = ELU(conv_k7(x)) and the pre-residual y = ELU(conv_k1(h)) (DESIGN.md gives the memory).
"""
from __future__ import annotations

import torch

from . import core, ops

F32 = torch.float32


def wants_grad(module, *tensors):
    """the one condition under which a graph is built: training mode, grad mode on, and an input or parameter that requires grad"""
    return module.training and torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters()))


class _ImageCache:
    """one derived weight image per module, rebuilt when the source tensors' (data_ptr, version) change -- like CausalConv1d.packed()"""

    def __init__(self):
        self._entry = None

    def get(self, tensors, make):
        ver = tuple((t.data_ptr(), core.tensor_version(t)) for t in tensors)
        if self._entry is None or self._entry[0] != ver:
            self._entry = (ver, make())
        return self._entry[1]


def conv_packed_t(mod):
    """transposed image of a CausalConv1d's weight for alm_conv1d_dgrad"""
    w = mod.conv.weight
    return mod._packed_t.get((w,), lambda: ops.conv1d_pack_t(w.detach().to(F32)))


def _conv_bwd(mod, g, y, x, need_x, need_w, residual=None):
    """(dx | None, dW | None, db | None) of one CausalConv1d given g = dL/dout (y: its saved post-ELU output or None)"""
    dx = dw = db = None
    if need_x:
        dx = ops.conv1d_dgrad(g, y, conv_packed_t(mod), x.shape[1], x.shape[2], mod.kernel_size, stride=mod.stride, dilation=mod.dilation, residual=residual)
    if need_w:
        dw, db = ops.conv1d_wgrad(g, y, x, mod.kernel_size, stride=mod.stride, dilation=mod.dilation)
    return dx, dw, db


class CausalConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod, elu):
        y = mod.run(x, elu=elu)
        ctx.mod, ctx.elu = mod, elu
        ctx.save_for_backward(x, weight, y if elu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        dx, dw, db = _conv_bwd(ctx.mod, g.to(F32).contiguous(), y, x, ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, dw, db, None, None


class ResidualUnitFn(torch.autograd.Function):
    """x + ELU(conv_k1(ELU(conv_k7(x))))"""

    @staticmethod
    def forward(ctx, x, w7, b7, w1, b1, unit):
        c7, c1 = unit.fn[0], unit.fn[2]
        h = c7.run(x, elu=True)
        y = c1.run(h, elu=True)
        ctx.unit = unit
        ctx.save_for_backward(x, h, y, w7, w1)
        return ops.add_f32(y, x)

    @staticmethod
    def backward(ctx, g):
        x, h, y, _, _ = ctx.saved_tensors
        c7, c1 = ctx.unit.fn[0], ctx.unit.fn[2]
        g = g.to(F32).contiguous()
        need7 = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need1 = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        dh, dw1, db1 = _conv_bwd(c1, g, y, h, ctx.needs_input_grad[0] or need7, need1)
        dx, dw7, db7 = _conv_bwd(c7, dh, h, x, ctx.needs_input_grad[0], need7, residual=g) if dh is not None else (None, None, None)
        return dx, dw7, db7, dw1, db1, None


class CausalConvTranspose1dFn(torch.autograd.Function):
    """the k = 2 zero-padded conv over s phase-major copies of the output channels + interleave; backward = de-interleave, then that conv's backward"""

    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        ctx.mod = mod
        ctx.save_for_backward(x, weight)
        return mod.run(x)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        mod = ctx.mod
        s, cout, cin = mod.upsample_factor, mod.conv.out_channels, mod.conv.in_channels
        gd = ops.phase_deinterleave(g.to(F32).contiguous(), cout, s)                          # [B, s * cout, n]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv1d_dgrad(gd, None, mod.packed_t(), cin, x.shape[2], 2, zero_pad=True)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw2, db2 = ops.conv1d_wgrad(gd, None, x, 2, zero_pad=True)                        # [(r, co), ci, tap]; tap 0 <-> w[ci, co, r + s], tap 1 <-> w[ci, co, r]
            dw2 = dw2.view(s, cout, cin, 2)
            dw = torch.cat((dw2[..., 1], dw2[..., 0]), dim=0).permute(2, 1, 0).contiguous()   # [cin, cout, 2 s]
            db = db2.view(s, cout).sum(0)
        return dx, dw, db, None


class BctToBtcFn(torch.autograd.Function):
    """'b c n -> b n c'; its adjoint is the same kernel with C and T exchanged"""

    @staticmethod
    def forward(ctx, x):
        return ops.bct_to_btc(x)

    @staticmethod
    def backward(ctx, g):
        return ops.bct_to_btc(g.to(F32).contiguous())
