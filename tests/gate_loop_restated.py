"""Plain-torch restatement of SoundStream's gate-loop layers (reference soundstream.py:314-330, 524-525, 620-621: after every EncoderBlock /
DecoderBlock one Residual(ChannelTranspose(GateLoop(c))), GateLoop = gateloop_transformer.SimpleGateLoopLayer), written from the formulas; runs on the
CPU in float32 or float64 and is differentiable by autograd.  The package is not installed here: parity with it is unpinned.  Test infrastructure:
nothing in the package imports it.

    r[b,t]   = sqrt(c) / max(||x[b,:,t]||_2, 1e-12)          RMSNorm over the channel axis (F.normalize's default eps)
    xn       = x * r * gamma[c]
    z        = W xn                                          W (3c, c): nn.Linear(c, 3c, bias=False).weight
    q, kv, a = z[0:c], z[c:2c], sigmoid(z[2c:3c])            'b n (qkva d)': qkva is the major index
    h[0]     = kv[0];  h[t] = a[t] h[t-1] + kv[t]            per (b, channel) row; a[0] is unused
    y        = q * h + 2 x                                   ChannelTranspose adds x, Residual adds x again
"""
import torch
import torch.nn.functional as F

import audiolm_oracle as O


def scan_loop(a, kv):
    """h[0] = kv[0]; h[t] = a[t] h[t-1] + kv[t] along the last axis, one step at a time"""
    hs = [kv[..., 0]]
    for t in range(1, kv.shape[-1]):
        hs.append(a[..., t] * hs[-1] + kv[..., t])
    return torch.stack(hs, dim=-1)


def scan_doubling(a, kv):
    """the same recurrence by log-step doubling of the maps h -> p h + s (Hillis-Steele): after the step of distance d, (p, s)[t] composes the
    steps t - 2 d + 1 .. t"""
    n = kv.shape[-1]
    p = torch.cat((torch.zeros_like(a[..., :1]), a[..., 1:]), dim=-1)          # a[0] is unused: the first map is the constant kv[0]
    s = kv
    d = 1
    while d < n:
        p_prev = F.pad(p[..., :-d], (d, 0), value=1.)                          # the identity map before the row's start
        s_prev = F.pad(s[..., :-d], (d, 0), value=0.)
        s = p * s_prev + s
        p = p * p_prev
        d *= 2
    return s


def gate_loop_parts(x, gamma, w):
    """x (b, c, n) -> (r (b, 1, n), xn, q, kv, a), the intermediate values named in the module docstring"""
    c = x.shape[1]
    r = (c ** 0.5) / x.norm(dim=1, keepdim=True).clamp(min=1e-12)
    xn = x * r * gamma[None, :, None]
    z = torch.einsum('oc,bcn->bon', w, xn)
    return r, xn, z[:, :c], z[:, c:2 * c], torch.sigmoid(z[:, 2 * c:])


def gate_loop_block(x, gamma, w, scan=scan_doubling):
    """x (b, c, n), gamma (c,), w (3c, c) -> q * h + 2 x"""
    _, _, q, kv, a = gate_loop_parts(x, gamma, w)
    return q * scan(a, kv) + 2 * x


def gate_loop_backward(x, gamma, w, g):
    """(dx, dgamma, dW, dz) of gate_loop_block given g = dL/dy, by the analytic formulas (no autograd): dq = g h; dh[n-1] = g q, dh[t] = g[t] q[t] +
    a[t+1] dh[t+1]; dkv = dh; dz_a[t] = dh[t] h[t-1] a (1 - a), 0 at t = 0; the projection's gradients; the RMSNorm backward; + 2 g"""
    c, n = x.shape[1], x.shape[2]
    r, xn, q, kv, a = gate_loop_parts(x, gamma, w)
    h = scan_loop(a, kv)
    gq = g * q
    dhs = [gq[..., n - 1]]
    for t in range(n - 2, -1, -1):
        dhs.append(gq[..., t] + a[..., t + 1] * dhs[-1])
    dh = torch.stack(dhs[::-1], dim=-1)
    h_prev = F.pad(h[..., :-1], (1, 0), value=0.)
    dza = dh * h_prev * a * (1 - a)
    dza[..., 0] = 0
    dz = torch.cat((g * h, dh, dza), dim=1)
    dw = torch.einsum('bon,bcn->oc', dz, xn)
    dxn = torch.einsum('oc,bon->bcn', w, dz)
    gm = gamma[None, :, None]
    dot = (dxn * gm * x).sum(dim=1, keepdim=True)
    dx = r * gm * dxn - x * (r ** 3 / c) * dot + 2 * g
    dgamma = (dxn * x * r).sum(dim=(0, 2))
    return dx, dgamma, dw, dz


def _block(sd, p, x):
    return gate_loop_block(x, sd[p + 'fn.fn.norm.gamma'], sd[p + 'fn.fn.to_qkva.0.weight'])


def encoder(sd, x, strides=(2, 4, 5, 8), dilations=(1, 3, 9), p='encoder.'):
    """the use_gate_loop_layers=True encoder stack: conv(k7) -> per stride [3 x ResidualUnit, strided conv(k = 2 s)], gate-loop block -> conv(k3);
    x (b, 1, n).  The blocks sit at indices 1, 3, 5, .. and the gate-loop blocks at 2, 4, 6, .."""
    x = O.causal_conv1d(x, sd[p + '0.conv.weight'], sd[p + '0.conv.bias'])
    for bi, s in enumerate(strides):
        bp = f'{p}{2 * bi + 1}.'
        for ri, d in enumerate(dilations):
            x = O.residual_unit(sd, f'{bp}{ri}.', x, d)
        x = O.causal_conv1d(x, sd[bp + '3.conv.weight'], sd[bp + '3.conv.bias'], stride=s)
        x = _block(sd, f'{p}{2 * bi + 2}.', x)
    last = 2 * len(strides) + 1
    return O.causal_conv1d(x, sd[f'{p}{last}.conv.weight'], sd[f'{p}{last}.conv.bias'])


def decoder(sd, x, strides=(2, 4, 5, 8), dilations=(1, 3, 9), p='decoder.'):
    """the use_gate_loop_layers=True decoder stack; x (b, c, n)"""
    x = O.causal_conv1d(x, sd[p + '0.conv.weight'], sd[p + '0.conv.bias'])
    for bi, s in enumerate(reversed(strides)):
        bp = f'{p}{2 * bi + 1}.'
        x = O.causal_conv_transpose1d(x, sd[bp + '0.conv.weight'], sd[bp + '0.conv.bias'], s)
        for ri, d in enumerate(dilations):
            x = O.residual_unit(sd, f'{bp}{ri + 1}.', x, d)
        x = _block(sd, f'{p}{2 * bi + 2}.', x)
    last = 2 * len(strides) + 1
    return O.causal_conv1d(x, sd[f'{p}{last}.conv.weight'], sd[f'{p}{last}.conv.bias'])


def autoencoder(sd, x, strides=(2, 4, 5, 8)):
    """decoder(encoder(x)) with no quantizer and no attention in between (use_local_attn=False): what `decode(encode(x))` computes"""
    return decoder(sd, encoder(sd, x, strides), strides)
