"""Autograd layer of the codec: `torch.autograd.Function`s over the backward kernels of csrc/codec_bwd.hip for CausalConv1d,
CausalConvTranspose1d and the ResidualUnit (reference soundstream.py:332-369), plus the layout transpose, and over csrc/local_attn_bwd.hip for the two
halves of a LocalTransformer layer (LocalMHA, feed-forward; soundstream.py:397-440).  soundstream.py takes them ONLY in training
mode with grad mode on and an input or parameter that requires grad; every other call issues the forward launches it always did.

The forward of each Function runs the SAME forward kernels as the eval path (the ResidualUnit as its two alm_conv1d_causal launches, to which the
fused alm_resunit_causal is bitwise equal, with the skip added by alm_add_f32), so a training-mode output is bitwise the eval-mode output.
Saved per ResidualUnit: its input x, the intermediate h = ELU(conv_k7(x)) and the pre-residual y = ELU(conv_k1(h)) (DESIGN.md gives the memory).
The squeeze-excite unit (ResidualUnitSEFn) and the FiLM conditioner (FiLMFn) run on csrc/film_se.hip the same way, the residual finite scalar
quantizer (FsqFn) on csrc/fsq.hip and the lookup-free quantizer (LfqFn) on csrc/lfq.hip.
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


def se_params(se):
    """(W1 [inner, C, 1], b1, W2 [C, inner, 1], b2) of a soundstream.SqueezeExcite as the kernels read them: the nn.Conv1d tensors themselves"""
    c1, c2 = se.net[0], se.net[2]
    return tuple(t.detach().to(F32).contiguous() for t in (c1.weight, c1.bias, c2.weight, c2.bias))


class ResidualUnitSEFn(torch.autograd.Function):
    """x + SE(ELU(conv_k1(ELU(conv_k7(x))))) (squeeze_excite=True): the eval path's three launches.  Saved: x, h = ELU(conv_k7(x)) and
    u = ELU(conv_k1(h)), the gate's input; the cumulative mean, the hidden layer and the gate are recomputed in alm_se_gate_bwd."""

    @staticmethod
    def forward(ctx, x, w7, b7, w1, b1, sw1, sb1, sw2, sb2, unit):
        c7, c1 = unit.fn[0], unit.fn[2]
        h = c7.run(x, elu=True)
        u = c1.run(h, elu=True)
        ctx.unit = unit
        ctx.save_for_backward(x, h, u, w7, w1, sw1, sb1, sw2, sb2)
        return ops.se_gate_fwd(u, *se_params(unit.fn[4]), residual=x)

    @staticmethod
    def backward(ctx, g):
        x, h, u = ctx.saved_tensors[:3]
        unit = ctx.unit
        c7, c1 = unit.fn[0], unit.fn[2]
        g = g.to(F32).contiguous()
        need = ctx.needs_input_grad
        need7, need1 = need[1] or need[2], need[3] or need[4]
        du, dsw1, dsb1, dsw2, dsb2 = ops.se_gate_bwd(g, u, *se_params(unit.fn[4]))
        dh, dw1, db1 = _conv_bwd(c1, du, u, h, need[0] or need7, need1)
        dx, dw7, db7 = _conv_bwd(c7, dh, h, x, need[0], need7, residual=g) if dh is not None else (None, None, None)
        return (dx, dw7, db7, dw1, db1, dsw1 if need[5] else None, dsb1 if need[6] else None, dsw2 if need[7] else None, dsb2 if need[8] else None, None)


class FiLMFn(torch.autograd.Function):
    """x * gamma + beta on (b, n, dim), (gamma | beta) = to_cond(cond) formed in the kernel; saved: x"""

    @staticmethod
    def forward(ctx, x, weight, bias, cond):
        ctx.cond = cond
        ctx.save_for_backward(x, weight, bias)
        return ops.film_fwd(x, weight.detach().to(F32).contiguous(), bias.detach().to(F32).contiguous(), *cond)

    @staticmethod
    def backward(ctx, g):
        x, weight, bias = ctx.saved_tensors
        dx, dw, db = ops.film_bwd(g.to(F32).contiguous(), x, weight.detach().to(F32).contiguous(), bias.detach().to(F32).contiguous(), *ctx.cond)
        need = ctx.needs_input_grad
        return dx if need[0] else None, dw if need[1] else None, db if need[2] else None, None


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


class RvqTrainFn(torch.autograd.Function):
    """one training step of the grouped residual VQ (soundstream.GroupedResidualVQ.train_step): x [M, dim] -> (out, losses [g, Q]; indices carry no
    gradient).  Saved: x, the indices [g, M, Q] and per group the step's PRE-update codebooks [Q, C, d]; every row's residual chain is recomputed in
    the backward (alm_rvq_train_bwd) instead of keeping Q residuals.  The codebooks get no gradient (EMA-trained)."""

    @staticmethod
    def forward(ctx, x, mod, k):
        out, losses, idx, snaps = mod.train_step(x, k)
        ctx.cfg = (mod.commitment_weight, mod.rotation_trick)
        ctx.save_for_backward(x, idx, *snaps)
        ctx.mark_non_differentiable(idx)
        return out, losses, idx

    @staticmethod
    def backward(ctx, g_out, g_losses, _):
        x, idx, *snaps = ctx.saved_tensors
        weight, rotation = ctx.cfg
        M, dim = x.shape
        dg = dim // len(snaps)
        g_out = g_out.to(F32).contiguous()
        dx = torch.empty_like(x)
        for gi, E in enumerate(snaps):
            coef = (g_losses[gi].to(F32) * (2. * weight / (M * dg))).contiguous()          # d loss_q / d r = 2 w (r - quant) / (M d)
            ops.rvq_train_bwd(x[:, gi * dg:(gi + 1) * dg], idx[gi], E, g_out[:, gi * dg:(gi + 1) * dg], coef, dx[:, gi * dg:(gi + 1) * dg], rotation)
        return dx, None, None


def _proj_quant_bwd(ctx, x, g_out, params, group_bwd):
    """the group loop of FsqFn.backward and LfqFn.backward.  group_bwd(g, g_out columns, x columns, kernel weights or None, dx columns) fills the dx
    columns and returns group g's parameter gradients (nothing in the identity case); returns what backward returns"""
    mod = ctx.mod
    dg = x.shape[1] // mod.groups
    g_out = g_out.to(F32).contiguous()
    dx = torch.empty_like(x)
    per = len(params) // mod.groups                                # 4, or 0 in the identity case
    grads = []
    for g in range(mod.groups):
        sl = slice(g * dg, (g + 1) * dg)
        grads.extend(group_bwd(g, g_out[:, sl], x[:, sl], mod.kernel_weights(params[per * g:per * g + per]), dx[:, sl]))
    need = ctx.needs_input_grad
    return (dx if need[0] else None, None, None, *[gr if need[3 + i] else None for i, gr in enumerate(grads)])


class FsqFn(torch.autograd.Function):
    """the grouped residual FSQ (soundstream.GroupedResidualFSQ.run): x [M, dim] -> (out, indices; the indices carry no gradient).  `params`: per
    group project_in.{weight, bias}, project_out.{weight, bias} (nothing in the identity case).  Saved: x, per group the projected input z [M, d] and
    the parameters; the chain is recomputed in alm_fsq_bwd, whose straight-through rounding and detached residual leave one direct path."""

    @staticmethod
    def forward(ctx, x, mod, k, *params):
        out, idx, zs = mod.run(x, k, save_z=True)
        ctx.mod, ctx.k = mod, k
        ctx.save_for_backward(x, *[z for z in zs if z is not None], *params)
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, g_out, _):
        mod, k = ctx.mod, ctx.k
        x, *rest = ctx.saved_tensors
        zs, params = (rest[:mod.groups], rest[mod.groups:]) if rest else ([None] * mod.groups, [])      # identity: neither z nor parameters
        consts = mod._consts(x.device)
        return _proj_quant_bwd(ctx, x, g_out, params, lambda g, go, xg, weights, dxg: ops.fsq_bwd(go, xg, zs[g], weights, consts, mod.proj_dim,
                                                                                                     mod.num_quantizers, k, dxg))


class LfqFn(torch.autograd.Function):
    """the grouped residual LFQ in training mode (soundstream.GroupedResidualLFQ.run): x [M, dim] -> (out, indices, losses [g, Q]; the indices carry
    no gradient, the losses do).  `params`: per group project_in.{weight, bias}, project_out.{weight, bias} (nothing in the identity case).  Saved: x,
    per group the projected input z [M, d] and the mean code distributions avg [Q, 2^d] (both float64), and the parameters; the chain and the softmax
    are recomputed in alm_lfq_bwd.  Every active layer is straight-through and the residual update detached: dz = (k + 1) g_z + the loss terms."""

    @staticmethod
    def forward(ctx, x, mod, k, *params):
        out, idx, losses, saved = mod.run(x, k, with_losses=True)
        ctx.mod, ctx.k = mod, k
        ctx.save_for_backward(x, *[t for pair in saved for t in pair], *params)
        ctx.mark_non_differentiable(idx)
        return out, idx, losses

    @staticmethod
    def backward(ctx, g_out, _, g_losses):
        mod, k = ctx.mod, ctx.k
        x, *rest = ctx.saved_tensors
        saved, params = rest[:2 * mod.groups], rest[2 * mod.groups:]
        g_losses = g_losses.to(F32).contiguous()
        return _proj_quant_bwd(ctx, x, g_out, params, lambda g, go, xg, weights, dxg: ops.lfq_bwd(
            go, g_losses[g], xg, saved[2 * g], saved[2 * g + 1], weights, mod.proj_dim, mod.num_quantizers, k, dxg, mod.loss_cfg))


# ---------------------------------------------------------------------------------------------- LocalTransformer (csrc/local_attn_bwd.hip)

def _lin_bwd(img, lin, g, x, need_x, need_w, residual=None):
    """(dx | None, dW | None, db | None) of an nn.Linear along the channel axis of [B, C, T] (a k = 1 conv; img: its soundstream._Linear1x1)"""
    dx = dw = db = None
    if need_x:
        dx = ops.conv1d_dgrad(g, None, img.packed_t(lin), x.shape[1], x.shape[2], 1, residual=residual)
    if need_w:
        dw, db = ops.conv1d_wgrad(g, None, x, 1)
        dw = dw.squeeze(-1)
        if lin.bias is None:
            db = None
    return dx, dw, db


class LocalMHAFn(torch.autograd.Function):
    """to_out(local_attn(to_qkv(LN(x)), gates = to_v_gate(LN(x)))) (+ x): the launches of LocalMHA.run.  Saved: x, LN(x), qkv, gates and the gated
    attention output o (2 dim + 4 H dh + H floats per frame); mean / rstd, the softmax statistics and the pre-gate output are recomputed."""

    @staticmethod
    def forward(ctx, x, norm_w, norm_b, w_qkv, q_scale, k_scale, w_gate, b_gate, w_out, mod, add_residual):
        xn, qkv, gates, o, y = mod.launches(x, add_residual)
        ctx.mod, ctx.add_residual = mod, add_residual
        ctx.save_for_backward(x, xn, qkv, gates, o, norm_w, w_qkv, q_scale, k_scale, w_gate, w_out)
        return y

    @staticmethod
    def backward(ctx, g):
        x, xn, qkv, gates, o, norm_w, _, q_scale, k_scale, _, _ = ctx.saved_tensors
        mod, need = ctx.mod, ctx.needs_input_grad
        l_qkv, l_gate, l_out = mod._lin
        g = g.to(F32).contiguous()
        do, dw_out, _ = _lin_bwd(l_out, mod.to_out, g, o, True, need[8])
        cos_t, sin_t, xpos_t = mod.tables(x.device)
        dqkv, dgates, dqs, dks = ops.local_attn_bwd(qkv, q_scale.detach().to(F32), k_scale.detach().to(F32), cos_t, sin_t, xpos_t, gates, o, do, mod.heads,
                                                    mod.dim_head, mod.window_size, mod.qk_scale)
        need_ln = need[0] or need[1] or need[2]
        dxn, dw_qkv, _ = _lin_bwd(l_qkv, mod.to_qkv, dqkv, xn, need_ln, need[3])
        dxn, dw_gate, db_gate = _lin_bwd(l_gate, mod.to_v_gate[0], dgates, xn, need_ln, need[6] or need[7], residual=dxn)      # dxn = both branches' sum
        dx = dgamma = dbeta = None
        if need_ln:
            dx, dgamma, dbeta = ops.layernorm_bct_bwd(dxn, x, norm_w.detach().to(F32), mod.norm.eps, residual=g if ctx.add_residual else None,
                                                      need_params=need[1] or need[2])
        return (dx if need[0] else None, dgamma, dbeta, dw_qkv, dqs if need[4] else None, dks if need[5] else None, dw_gate, db_gate, dw_out, None, None)


class LocalFeedForwardFn(torch.autograd.Function):
    """W2(GEGLU(W1(LN(x)))) + x: the launches of LocalTransformer's feed-forward half.  Saved: x, LN(x), the pre-activation u = W1 LN(x) and
    h = GEGLU(u) (2 dim + 3 I floats per frame)."""

    @staticmethod
    def forward(ctx, x, norm_w, norm_b, w1, w2, ff, lins):
        xn, u, h, y = ff_launches(ff, lins, x)
        ctx.ff, ctx.lins = ff, lins
        ctx.save_for_backward(x, xn, u, h, norm_w, w1, w2)
        return y

    @staticmethod
    def backward(ctx, g):
        x, xn, u, h, norm_w, _, _ = ctx.saved_tensors
        ff, lins, need = ctx.ff, ctx.lins, ctx.needs_input_grad
        g = g.to(F32).contiguous()
        dh, dw2, _ = _lin_bwd(lins[1], ff[4], g, h, True, need[4])
        du = ops.geglu_bct_bwd(dh, u)
        need_ln = need[0] or need[1] or need[2]
        dxn, dw1, _ = _lin_bwd(lins[0], ff[1], du, xn, need_ln, need[3])
        dx = dgamma = dbeta = None
        if need_ln:
            dx, dgamma, dbeta = ops.layernorm_bct_bwd(dxn, x, norm_w.detach().to(F32), ff[0].eps, residual=g, need_params=need[1] or need[2])
        return dx if need[0] else None, dgamma, dbeta, dw1, dw2, None, None


class GateLoopFn(torch.autograd.Function):
    """the gate-loop block q * h + 2 x (soundstream.Residual.launches).  Saved: x and z = to_qkva(RMSNorm(x)) (4 dim floats per frame, 16 bytes per
    element of x); RMSNorm(x) and the state h are recomputed in the backward (one launch each: 8 bytes per element less than keeping them)."""

    @staticmethod
    def forward(ctx, x, gamma, weight, block):
        z, y = block.launches(x)
        ctx.block = block
        ctx.save_for_backward(x, z, gamma, weight)
        return y

    @staticmethod
    def backward(ctx, g):
        x, z, gamma, _ = ctx.saved_tensors
        layer, need = ctx.block.layer, ctx.needs_input_grad
        g = g.to(F32).contiguous()
        gamma = gamma.detach().to(F32).contiguous()
        dz = ops.gate_loop_scan_bwd(g, z, ops.gate_loop_scan_fwd(z))
        xn = ops.gate_loop_norm_fwd(x, gamma) if need[2] else x          # only the weight gradient reads xn's values
        dxn, dw, _ = _lin_bwd(layer._lin, layer.to_qkva[0], dz, xn, True, need[2])
        dx, dgamma = ops.gate_loop_norm_bwd(dxn, x, gamma, g)
        return dx if need[0] else None, dgamma if need[1] else None, dw, None


def ff_launches(ff, lins, x):
    """(LN(x), u, GEGLU(u), W2 GEGLU(u) + x) of one feed-forward block (ff: the Sequential, lins: its two soundstream._Linear1x1)"""
    xn = ops.layernorm_bct(x, ff[0].weight.detach(), ff[0].bias.detach(), ff[0].eps)
    u = lins[0](ff[1], xn)
    h = ops.geglu_bct(u)
    return xn, u, h, lins[1](ff[4], h, residual=x)
