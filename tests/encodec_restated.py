"""The causal 24 kHz EnCodec model (SEANet encoder / decoder with weight-normed convs, a 2-layer LSTM with a skip, a residual VQ) restated in plain torch,
any dtype, from a state dict under the transformers `EncodecModel` key names.  Oracle of tests/test_gpu_encodec.py; pinned to
`transformers.models.encodec.modeling_encodec.EncodecModel` in fp64 by tests/golden/make_encodec_golden.py -> tests/golden/encodec_tiny.pt
(tests/test_encodec_host.py compares to 1e-10).  Does not import transformers or the package under test.

Layout of the model (EncodecEncoder / EncodecDecoder):
  encoder.layers: 0 conv(1 -> F, k)  | per ratio r of reversed(ratios): resblock(s) , ELU , conv(c -> 2 c, 2 r, stride r) | lstm , ELU , conv(-> hidden, k_last)
  decoder.layers: 0 conv(hidden -> 16 F, k) , lstm | per ratio r: ELU , convtr(c -> c / 2, 2 r, stride r) , resblock(s) | ELU , conv(F -> 1, k_last)
  resblock(x) = shortcut_1x1(x) + conv_1x1(ELU(conv_k3,dil(ELU(x))))
Every conv is causal: reflect left pad of (k - 1) dil + 1 - stride, reflect right pad up to the next multiple of the stride.  The transposed conv keeps
the first n * stride outputs.
"""
import math

import torch
import torch.nn.functional as F

DEFAULTS = dict(num_filters=32, upsampling_ratios=(8, 5, 4, 2), hidden_size=128, codebook_size=1024, num_lstm_layers=2, kernel_size=7,
                last_kernel_size=7, residual_kernel_size=3, num_residual_layers=1, dilation_growth_rate=2, compress=2, use_conv_shortcut=True,
                sampling_rate=24000, num_codebooks=32)


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    c['upsampling_ratios'] = tuple(c['upsampling_ratios'])
    return c


def hop(cfg):
    return math.prod(cfg['upsampling_ratios'])


def num_quantizers(bandwidth, cfg):
    frame_rate = math.ceil(cfg['sampling_rate'] / hop(cfg))
    return int(max(1, math.floor(bandwidth * 1000 / (math.log2(cfg['codebook_size']) * frame_rate))))


def layout(cfg):
    """(encoder, decoder): lists of (kind, layer index, ...) in execution order; 'elu' entries carry no weights"""
    Fn, k, kl = cfg['num_filters'], cfg['kernel_size'], cfg['last_kernel_size']
    enc, i, c = [('conv', 0, 1, Fn, k, 1, 1)], 1, Fn
    for r in reversed(cfg['upsampling_ratios']):
        for j in range(cfg['num_residual_layers']):
            enc.append(('res', i, c, cfg['dilation_growth_rate'] ** j))
            i += 1
        enc += [('elu', i), ('conv', i + 1, c, 2 * c, 2 * r, r, 1)]
        i, c = i + 2, 2 * c
    enc += [('lstm', i, c), ('elu', i + 1), ('conv', i + 2, c, cfg['hidden_size'], kl, 1, 1)]
    dec, i = [('conv', 0, cfg['hidden_size'], c, k, 1, 1), ('lstm', 1, c)], 2
    for r in cfg['upsampling_ratios']:
        dec += [('elu', i), ('convtr', i + 1, c, c // 2, r)]
        i, c = i + 2, c // 2
        for j in range(cfg['num_residual_layers']):
            dec.append(('res', i, c, cfg['dilation_growth_rate'] ** j))
            i += 1
    dec += [('elu', i), ('conv', i + 1, c, 1, kl, 1, 1)]
    return enc, dec


def _shapes(cfg):
    """key -> shape of every weight tensor, transformers names (weight norm as parametrizations.weight.original0 / original1)"""
    out = {}

    def conv(p, cin, cout, k, transposed=False):
        w = (cin, cout, k) if transposed else (cout, cin, k)
        out[p + '.conv.parametrizations.weight.original0'] = (w[0], 1, 1)
        out[p + '.conv.parametrizations.weight.original1'] = w
        out[p + '.conv.bias'] = (cout,)

    for side, lay in zip(('encoder', 'decoder'), layout(cfg)):
        for e in lay:
            p = f'{side}.layers.{e[1]}'
            if e[0] == 'conv':
                conv(p, e[2], e[3], e[4])
            elif e[0] == 'convtr':
                conv(p, e[2], e[3], 2 * e[4], transposed=True)
            elif e[0] == 'res':
                dim, hid = e[2], e[2] // cfg['compress']
                conv(p + '.block.1', dim, hid, cfg['residual_kernel_size'])
                conv(p + '.block.3', hid, dim, 1)
                if cfg['use_conv_shortcut']:
                    conv(p + '.shortcut', dim, dim, 1)
            elif e[0] == 'lstm':
                for l in range(cfg['num_lstm_layers']):
                    out[f'{p}.lstm.weight_ih_l{l}'] = out[f'{p}.lstm.weight_hh_l{l}'] = (4 * e[2], e[2])
                    out[f'{p}.lstm.bias_ih_l{l}'] = out[f'{p}.lstm.bias_hh_l{l}'] = (4 * e[2],)
    return out


def _get(sd, prefix, a, b):
    return sd[prefix + a] if prefix + a in sd else sd[prefix + b]


def folded(sd, p, dtype):
    """w = g v / |v|, the norm over every axis but 0 (for the transposed conv's [Cin, Cout, k] weight axis 0 is the input channel)"""
    g = _get(sd, p + '.conv.', 'parametrizations.weight.original0', 'weight_g').to(dtype)
    v = _get(sd, p + '.conv.', 'parametrizations.weight.original1', 'weight_v').to(dtype)
    return g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)


def conv(sd, p, x, stride=1, dil=1):
    w, b = folded(sd, p, x.dtype), sd[p + '.conv.bias'].to(x.dtype)
    k = (w.shape[-1] - 1) * dil + 1
    left, T = k - stride, x.shape[-1]
    right = (math.ceil((T - k + left) / stride + 1) - 1) * stride + k - left - T
    if T <= max(left, right):
        raise ValueError(f'{T} steps are too few for a reflect pad of {max(left, right)}')
    return F.conv1d(F.pad(x, (left, right), mode='reflect'), w, b, stride=stride, dilation=dil)


def convtr(sd, p, x, stride):
    w, b = folded(sd, p, x.dtype), sd[p + '.conv.bias'].to(x.dtype)
    return F.conv_transpose1d(x, w, b, stride=stride)[..., :x.shape[-1] * stride]


def lstm(sd, p, x, layers):
    """x [B, C, T] -> lstm(x) + x, same layout (zero initial state, gate order i f g o)"""
    m = torch.nn.LSTM(x.shape[1], x.shape[1], layers).to(x.dtype)
    m.load_state_dict({k[len(p) + 6:]: v.to(x.dtype) for k, v in sd.items() if k.startswith(p + '.lstm.')})
    s = x.permute(2, 0, 1)
    with torch.no_grad():
        return (m(s)[0] + s).permute(1, 2, 0)


def _run(sd, side, lay, x, cfg):
    for e in lay:
        p = f'{side}.layers.{e[1]}'
        if e[0] == 'elu':
            x = F.elu(x)
        elif e[0] == 'conv':
            x = conv(sd, p, x, e[5], e[6])
        elif e[0] == 'convtr':
            x = convtr(sd, p, x, e[4])
        elif e[0] == 'lstm':
            x = lstm(sd, p, x, cfg['num_lstm_layers'])
        else:
            h = conv(sd, p + '.block.1', F.elu(x), 1, e[3])
            h = conv(sd, p + '.block.3', F.elu(h))
            x = (conv(sd, p + '.shortcut', x) if cfg['use_conv_shortcut'] else x) + h
    return x


@torch.no_grad()
def encoder(sd, wave, dtype=torch.float64, **cfg):
    """wave [B, T] -> features [B, ceil(T / hop), hidden]"""
    cfg = config(**cfg)
    return _run(sd, 'encoder', layout(cfg)[0], wave.to(dtype)[:, None], cfg).transpose(1, 2)


def codebooks(sd, n_q, dtype=torch.float64):
    return torch.stack([sd[f'quantizer.layers.{q}.codebook.embed'].to(dtype) for q in range(n_q)])


def distances(r, E):
    """the (negated) score EncodecEuclideanCodebook.quantize maximises: |r|^2 - 2 r.e + |e|^2, [.., C]"""
    return r.pow(2).sum(-1, keepdim=True) - 2 * r @ E.t() + E.pow(2).sum(-1)


@torch.no_grad()
def codes(sd, feats, n_q):
    """feats [B, n, d] -> codes [B, n, n_q] int64: nearest code (first index on ties), residual passed on"""
    E, r, out = codebooks(sd, n_q, feats.dtype), feats, []
    for q in range(n_q):
        idx = (-distances(r, E[q])).max(dim=-1).indices
        out.append(idx)
        r = r - E[q][idx]
    return torch.stack(out, dim=-1)


@torch.no_grad()
def emb(sd, code, dtype=torch.float64):
    """codes [B, n, q] -> sum of the code vectors [B, n, d]"""
    E = codebooks(sd, code.shape[-1], dtype)
    return sum(E[q][code[..., q]] for q in range(code.shape[-1]))


@torch.no_grad()
def decoder(sd, e, **cfg):
    """[B, n, d] -> wave [B, 1, n * hop]"""
    cfg = config(**cfg)
    return _run(sd, 'decoder', layout(cfg)[1], e.transpose(1, 2), cfg)


def decode(sd, code, dtype=torch.float64, **cfg):
    return decoder(sd, emb(sd, code, dtype), **cfg)


def random_state_dict(seed, zero_bias=False, **cfg):
    """seeded weights under the transformers names.  v ~ N(0, 1 / fan_in), g = |v| (1 + 0.1 N), biases 0.1 N (or zero: with the default-size model
    non-zero biases dominate the features and most frames look alike), LSTM U(-1 / sqrt(H), 1 / sqrt(H)).  transformers initialises the codebooks to
    zero; here level q holds rows drawn from the fp64 level-q residuals of 4 other seeded clips plus noise of one residual standard deviation."""
    cfg = config(**cfg)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    trs = {f'decoder.layers.{e[1]}' for e in layout(cfg)[1] if e[0] == 'convtr'}     # [Cin, Cout, 2 s]: two taps of every input channel per output
    for k, shape in _shapes(cfg).items():
        if k.endswith('original0'):
            continue
        if k.endswith('original1'):
            transposed = k.split('.conv.')[0] in trs
            fan_in = 2 * shape[0] if transposed else shape[1] * shape[2]
            v = torch.randn(shape, generator=g) * fan_in ** -0.5
            sd[k[:-1] + '0'] = v.flatten(1).norm(dim=1).view(-1, 1, 1) * (1 + 0.1 * torch.randn(shape[0], 1, 1, generator=g))
            sd[k] = v
        elif '.bias' in k and zero_bias:
            sd[k] = torch.zeros(shape)
        elif '.lstm.' in k:
            sd[k] = (torch.rand(shape, generator=g) * 2 - 1) * shape[-1] ** -0.5
        else:
            sd[k] = 0.1 * torch.randn(shape, generator=g)
    C, Q = cfg['codebook_size'], cfg['num_codebooks']
    clips = torch.randn(4, hop(cfg) * max(math.ceil(C / 4), 8), generator=g) * 0.3
    r = encoder(sd, clips, torch.float64, **cfg).reshape(-1, cfg['hidden_size'])
    for q in range(Q):
        E = (r[torch.randperm(r.shape[0], generator=g)[:C]] + r.std() * torch.randn(C, r.shape[1], generator=g, dtype=torch.float64)).float()
        sd[f'quantizer.layers.{q}.codebook.embed'] = E
        r = r - E.double()[(-distances(r, E.double())).max(dim=-1).indices]
    return sd


class _Quantizer:
    def __init__(self, sd, dtype):
        self.sd, self.dtype = sd, dtype

    def decode(self, code):                                        # [q, b, n] -> [b, d, n]
        return emb(self.sd, code.permute(1, 2, 0), self.dtype).transpose(1, 2)


class Model:
    """what the reference's EncodecWrapper touches of Meta's EncodecModel: .channels, .sample_rate, .segment_stride, .training,
    .encode(wav [b, 1, t]) -> [(codes [b, q, n], None)], .quantizer.decode(codes [q, b, n]) -> [b, d, n], .decoder([b, d, n]) -> [b, 1, t]"""

    def __init__(self, sd, bandwidth=6.0, dtype=torch.float64, **cfg):
        self.sd, self.cfg, self.dtype = sd, config(**cfg), dtype
        self.channels, self.sample_rate, self.segment_stride, self.training = 1, self.cfg['sampling_rate'], None, False
        self.n_q = num_quantizers(bandwidth, self.cfg)
        self.quantizer = _Quantizer(sd, dtype)

    def encode(self, wav):
        f = encoder(self.sd, wav[:, 0], self.dtype, **self.cfg)
        return [(codes(self.sd, f, self.n_q).transpose(1, 2), None)]

    def decoder(self, e):
        return decoder(self.sd, e.transpose(1, 2).to(self.dtype), **self.cfg)
