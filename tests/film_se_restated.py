"""Plain-torch restatement of the denoising SoundStream's two extra pieces, written from their formulas (reference soundstream.py:145-169, 362-369,
442-449); runs on the CPU in float32 or float64 and is differentiable by autograd.  Test infrastructure: nothing in the package imports it.

    FiLM            gamma, beta = (W cond + b).chunk(2);  y = x * gamma + beta                          x (b, n, dim), W (2 dim, 2)
    SqueezeExcite   inside a ResidualUnit the input is (b, c, n) and the module takes shape[-2] and cumsum(dim=-2): the cumulative mean runs over
                    the CHANNEL axis, m[c] = (u[0] + .. + u[c]) / (c + 1) per time step; gate = sigmoid(W2 silu(W1 m + b1) + b2); y = u * gate
    SE unit         x + SE(ELU(conv_k1(ELU(conv_k7(x)))))
"""
import torch
import torch.nn.functional as F

import audiolm_oracle as O


def film(x, w, b, cond):
    """x (..., dim), w (2 dim, 2), b (2 dim), cond (2,) -> x * gamma + beta"""
    gamma, beta = (w @ cond.to(w.dtype) + b).chunk(2, dim=-1)
    return x * gamma + beta


def cond_of(is_denoising, dtype=torch.float32):
    return torch.tensor([float(bool(is_denoising)), float(not is_denoising)], dtype=dtype)


def channel_cumulative_mean(u):
    """u (b, c, n) -> m[c] = mean(u[0..c]) as the product with the lower-triangular-mean matrix L[c][c'] = (c' <= c) / (c + 1)"""
    C = u.shape[-2]
    return u.cumsum(dim=-2) / torch.arange(1, C + 1, dtype=u.dtype, device=u.device)[:, None]


def squeeze_excite(u, w1, b1, w2, b2):
    """u (b, c, n), w1 (inner, c, 1), w2 (c, inner, 1) -> u * gate"""
    m = channel_cumulative_mean(u)
    hidden = F.silu(F.conv1d(m, w1, b1))
    return u * torch.sigmoid(F.conv1d(hidden, w2, b2))


def se_residual_unit(sd, p, x, dilation):
    h = F.elu(O.causal_conv1d(x, sd[p + 'fn.0.conv.weight'], sd[p + 'fn.0.conv.bias'], dilation=dilation))
    u = F.elu(O.causal_conv1d(h, sd[p + 'fn.2.conv.weight'], sd[p + 'fn.2.conv.bias']))
    return x + squeeze_excite(u, sd[p + 'fn.4.net.0.weight'], sd[p + 'fn.4.net.0.bias'], sd[p + 'fn.4.net.2.weight'], sd[p + 'fn.4.net.2.bias'])


def encoder(sd, x, strides=(2, 4, 5, 8), dilations=(1, 3, 9), p='encoder.'):
    """the squeeze_excite=True encoder stack: conv(k7) -> per stride [3 x SE unit, strided conv(k = 2 s)] -> conv(k3); x (b, 1, n)"""
    x = O.causal_conv1d(x, sd[p + '0.conv.weight'], sd[p + '0.conv.bias'])
    for bi, s in enumerate(strides):
        bp = f'{p}{bi + 1}.'
        for ri, d in enumerate(dilations):
            x = se_residual_unit(sd, f'{bp}{ri}.', x, d)
        x = O.causal_conv1d(x, sd[bp + '3.conv.weight'], sd[bp + '3.conv.bias'], stride=s)
    last = len(strides) + 1
    return O.causal_conv1d(x, sd[f'{p}{last}.conv.weight'], sd[f'{p}{last}.conv.bias'])


def decoder(sd, x, strides=(2, 4, 5, 8), dilations=(1, 3, 9), p='decoder.'):
    """the squeeze_excite=True decoder stack; x (b, c, n)"""
    x = O.causal_conv1d(x, sd[p + '0.conv.weight'], sd[p + '0.conv.bias'])
    for bi, s in enumerate(reversed(strides)):
        bp = f'{p}{bi + 1}.'
        x = O.causal_conv_transpose1d(x, sd[bp + '0.conv.weight'], sd[bp + '0.conv.bias'], s)
        for ri, d in enumerate(dilations):
            x = se_residual_unit(sd, f'{bp}{ri + 1}.', x, d)
    last = len(strides) + 1
    return O.causal_conv1d(x, sd[f'{p}{last}.conv.weight'], sd[f'{p}{last}.conv.bias'])


def denoising_autoencoder(sd, x, is_denoising, strides=(2, 4, 5, 8)):
    """y = decoder(decoder_film(encoder_film(encoder(x)^T))^T) with no quantizer in between: the composition of tests/golden/film_se_small.pt"""
    cond = cond_of(is_denoising, x.dtype)
    f = encoder(sd, x, strides).transpose(1, 2)
    f = film(f, sd['encoder_film.to_cond.weight'], sd['encoder_film.to_cond.bias'], cond)
    f = film(f, sd['decoder_film.to_cond.weight'], sd['decoder_film.to_cond.bias'], cond)
    return decoder(sd, f.transpose(1, 2), strides)


def golden_grads(entry):
    """one condition's entry of tests/golden/film_se_small.pt -> {name: (shape, stride, reference values of flat[::stride])}"""
    flat = entry['grad_flat']
    return {k: (tuple(shape), stride, flat[off:off + n]) for k, shape, stride, off, n in entry['grad_index']}
