"""The fairseq HuBERT-base feature model and the reference's k-means assignment, restated in plain torch as test infrastructure.

fairseq is not available to this project.  This is the oracle that audiolm-pytorch_amd/hubert_kmeans.py + csrc/hubert.hip are checked against; it is
written from the published architecture (group-norm conv feature extractor, LayerNorm + Linear, weight-normed grouped positional conv with the last
sample dropped, post-LN encoder layers), runs from a fairseq-named state dict and nothing here imports the product.  `dtype` selects the arithmetic:
fp32 is what fairseq computes, fp64 the high-precision yardstick.  tests/test_hubert_host.py pins it to transformers.HubertModel in fp64.
"""
import math

import torch
import torch.nn.functional as F

BASE_CONV = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
# gain of the value / output / fc2 weights of random_state_dict: fairseq initialises its Linear weights with std 0.02, a gain of 0.02 sqrt(768) = 0.55 at
# base width, so the residual stream keeps each frame's identity through the layers (gain 1 lets the attention average wash the frames into one point)
BRANCH_GAIN = 0.55


def frame_count(T, conv=BASE_CONV):
    for _, k, s in conv:
        T = (T - k) // s + 1
    return T


def random_state_dict(seed, dim=768, layers=9, ffn=None, conv=BASE_CONV, conv_pos=128, groups=16, extra_layers=0, dtype=torch.float32):
    """seeded fairseq-named weights with sensible scales (activations stay O(1) through the stack)"""
    g = torch.Generator().manual_seed(seed)
    ffn = ffn or 4 * dim

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)
    sd = {}
    cin = 1
    for i, (c, k, s) in enumerate(conv):
        sd[f'feature_extractor.conv_layers.{i}.0.weight'] = rn(c, cin, k, scale=math.sqrt(2.0 / (cin * k)))
        cin = c
    sd['feature_extractor.conv_layers.0.2.weight'] = 1 + rn(conv[0][0], scale=0.1)
    sd['feature_extractor.conv_layers.0.2.bias'] = rn(conv[0][0], scale=0.1)
    sd['layer_norm.weight'] = 1 + rn(cin, scale=0.1)
    sd['layer_norm.bias'] = rn(cin, scale=0.1)
    sd['post_extract_proj.weight'] = rn(dim, cin, scale=cin ** -0.5)
    sd['post_extract_proj.bias'] = rn(dim, scale=0.1)
    sd['encoder.pos_conv.0.weight_v'] = rn(dim, dim // groups, conv_pos, scale=1.0)
    sd['encoder.pos_conv.0.weight_g'] = (rn(1, 1, conv_pos, scale=0.1).abs() + 1.0) * math.sqrt(dim / groups) * 0.5
    sd['encoder.pos_conv.0.bias'] = rn(dim, scale=0.1)
    sd['encoder.layer_norm.weight'] = 1 + rn(dim, scale=0.1)
    sd['encoder.layer_norm.bias'] = rn(dim, scale=0.1)
    for i in range(layers + extra_layers):
        p = f'encoder.layers.{i}.'
        for n in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            sd[p + f'self_attn.{n}.weight'] = rn(dim, dim, scale=(2.0 if n in ('q_proj', 'k_proj') else BRANCH_GAIN) * dim ** -0.5)
            sd[p + f'self_attn.{n}.bias'] = rn(dim, scale=0.1)
        sd[p + 'fc1.weight'] = rn(ffn, dim, scale=dim ** -0.5)
        sd[p + 'fc1.bias'] = rn(ffn, scale=0.1)
        sd[p + 'fc2.weight'] = rn(dim, ffn, scale=BRANCH_GAIN * ffn ** -0.5)
        sd[p + 'fc2.bias'] = rn(dim, scale=0.1)
        for n in ('self_attn_layer_norm', 'final_layer_norm'):
            sd[p + n + '.weight'] = 1 + rn(dim, scale=0.1)
            sd[p + n + '.bias'] = rn(dim, scale=0.1)
    return sd


def gelu(x):
    return F.gelu(x)            # erf form


def conv0_groupnorm_gelu(wave, w, gamma, beta, stride, dtype, eps=1e-5):
    """layer 0: conv(1 -> C) + GroupNorm(C, C) (per row and channel over time, biased variance) + GELU; wave [B, T] -> [B, C, T0]"""
    c = F.conv1d(wave.to(dtype)[:, None], w.to(dtype), stride=stride)
    return gelu(F.group_norm(c, c.shape[1], gamma.to(dtype), beta.to(dtype), eps))


def pos_conv(x, weight_g, weight_v, bias, groups, dtype):
    """x [B, D, n] -> x + gelu(conv(x)) with w = g v / |v| (norm over all but the tap axis), padding k // 2, last output dropped for an even k"""
    g, v = weight_g.to(dtype), weight_v.to(dtype)
    w = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    k = w.shape[-1]
    y = F.conv1d(x, w, bias.to(dtype), padding=k // 2, groups=groups)
    if k % 2 == 0:
        y = y[..., :-1]
    return x + gelu(y)


def attention(q, k, v, heads):
    """q, k, v [B, n, D] (q unscaled) -> [B, n, D]; q is scaled by head_dim ** -0.5 before the product, as fairseq does"""
    B, n, D = q.shape
    dh = D // heads
    q = (q * dh ** -0.5).view(B, n, heads, dh).transpose(1, 2)
    k = k.view(B, n, heads, dh).transpose(1, 2)
    v = v.view(B, n, heads, dh).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, n, D)


def features(sd, wave, layers=9, heads=None, conv=BASE_CONV, groups=16, dtype=torch.float32):
    """wave [B, T] -> [B, n, D]: model(wave, features_only=True, mask=False, output_layer=layers)['x']"""
    W = lambda name: sd[name].to(dtype)
    x = conv0_groupnorm_gelu(wave, sd['feature_extractor.conv_layers.0.0.weight'], sd['feature_extractor.conv_layers.0.2.weight'],
                             sd['feature_extractor.conv_layers.0.2.bias'], conv[0][2], dtype)
    for i, (_, _, s) in enumerate(conv[1:], 1):
        x = gelu(F.conv1d(x, W(f'feature_extractor.conv_layers.{i}.0.weight'), stride=s))
    x = x.transpose(1, 2)
    x = F.layer_norm(x, x.shape[-1:], W('layer_norm.weight'), W('layer_norm.bias'), 1e-5)
    x = F.linear(x, W('post_extract_proj.weight'), W('post_extract_proj.bias'))
    D = x.shape[-1]
    heads = heads or D // 64
    x = pos_conv(x.transpose(1, 2), sd['encoder.pos_conv.0.weight_g'], sd['encoder.pos_conv.0.weight_v'], sd['encoder.pos_conv.0.bias'], groups,
                 dtype).transpose(1, 2)
    x = F.layer_norm(x, (D,), W('encoder.layer_norm.weight'), W('encoder.layer_norm.bias'), 1e-5)
    for i in range(layers):
        p = f'encoder.layers.{i}.'
        lin = lambda t, n: F.linear(t, W(p + n + '.weight'), W(p + n + '.bias'))
        a = attention(lin(x, 'self_attn.q_proj'), lin(x, 'self_attn.k_proj'), lin(x, 'self_attn.v_proj'), heads)
        x = x + lin(a, 'self_attn.out_proj')
        x = F.layer_norm(x, (D,), W(p + 'self_attn_layer_norm.weight'), W(p + 'self_attn_layer_norm.bias'), 1e-5)
        x = x + lin(gelu(lin(x, 'fc1')), 'fc2')
        x = F.layer_norm(x, (D,), W(p + 'final_layer_norm.weight'), W(p + 'final_layer_norm.bias'), 1e-5)
    return x


class Model:
    """stands in for the fairseq model object inside the reference's HubertWithKmeans.forward: called as
    model(wav, features_only=True, mask=False, output_layer=L) -> {'x': features}"""

    def __init__(self, sd, heads=None, conv=BASE_CONV, groups=16, dtype=torch.float32):
        self.sd, self.heads, self.conv, self.groups, self.dtype = sd, heads, conv, groups, dtype

    def eval(self):
        return self

    def __call__(self, wav, features_only=True, mask=False, output_layer=None, padding_mask=None):
        assert features_only and not mask and padding_mask is None
        return {'x': features(self.sd, wav, output_layer, self.heads, self.conv, self.groups, self.dtype)}


def assign(embed, centres):
    """(-cdist(embed, centres)).argmax(-1): nearest centre, first index on ties"""
    return (-torch.cdist(embed, centres.to(embed.dtype)[None].expand(embed.shape[0], -1, -1), p=2)).argmax(dim=-1)


def distances(embed, centres):
    """exact pairwise distances by differences (no |x|^2 + |c|^2 - 2 x.c cancellation), [B, n, C]"""
    return (embed[:, :, None, :] - centres.to(embed.dtype)[None, None]).pow(2).sum(-1).sqrt()
