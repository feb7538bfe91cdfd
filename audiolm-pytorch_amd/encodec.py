"""EncodecWrapper on the MI355X: the causal 24 kHz EnCodec model -- wave -> codes -> wave (reference encodec.py:25-177) -- without Meta's `encodec`
package and without ever resolving a hub name: the weights come from a local file or a state dict.

  wave [B, T] -> conv(1 -> F, k 7) -> per ratio r of (2, 4, 5, 8): resblock, ELU, conv(c -> 2 c, k 2 r, stride r)      alm_conv1d_causal_pre
              -> lstm(x) + x (2 layers) -> ELU -> conv(-> 128, k 7)                                                  alm_conv1d_valid + alm_lstm_seq
              -> 'b c n -> b n c' -> residual VQ, `num_quantizers` of the 32 codebooks                                alm_bct_to_btc, alm_rvq_encode
  codes -> summed code vectors -> conv(128 -> 16 F, k 7) -> lstm(x) + x                                              alm_rvq_decode
        -> per ratio r of (8, 5, 4, 2): ELU, transposed conv(c -> c / 2, k 2 r, stride r), resblock -> ELU -> conv(F -> 1, k 7)
  resblock(x) = shortcut_1x1(x) + conv_1x1(ELU(conv_k3(ELU(x))));  every conv is causal (reflect left pad) and weight-normed (folded once at load).

Parameters are registered under the transformers `EncodecModel` key names (weight norm in the weight_g / weight_v spelling; the
parametrizations.weight.original0 / original1 spelling loads too), so `EncodecModel.state_dict()` loads by name; `meta_to_hf_state_dict` renames a
checkpoint of Meta's package.  Everything outside the causal weight-norm mono model raises NotImplementedError; a CPU tensor raises RuntimeError.
"""
from __future__ import annotations

import functools
import math
import os
import re

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .frozen import F32, FrozenModel, load_weights
from .resample import resample

_IGNORED = re.compile(r'^quantizer\.layers\.\d+\.codebook\.(inited|cluster_size|embed_avg)$')
_CONFIG = dict(num_filters=32, upsampling_ratios=(8, 5, 4, 2), hidden_size=128, codebook_size=1024, num_lstm_layers=2, kernel_size=7, last_kernel_size=7,
               residual_kernel_size=3, num_residual_layers=1, dilation_growth_rate=2, compress=2, use_conv_shortcut=True, sampling_rate=24000)
_UNSUPPORTED = dict(norm_type='weight_norm', use_causal_conv=True, normalize=False, chunk_length_s=None, audio_channels=1, trim_right_ratio=1, pad_mode='reflect')


def _layout(cfg):
    """(encoder, decoder) of EncodecEncoder / EncodecDecoder as lists of ('conv', index, cin, cout, k, stride) | ('convtr', index, cin, cout, stride) |
    ('res', index, dim, dilation) | ('lstm', index, dim) | ('elu', index) in execution order; index = position in `.layers`"""
    Fn = cfg['num_filters']
    enc, i, c = [('conv', 0, 1, Fn, cfg['kernel_size'], 1)], 1, Fn
    for r in reversed(cfg['upsampling_ratios']):
        for j in range(cfg['num_residual_layers']):
            enc.append(('res', i, c, cfg['dilation_growth_rate'] ** j))
            i += 1
        enc += [('elu', i), ('conv', i + 1, c, 2 * c, 2 * r, r)]
        i, c = i + 2, 2 * c
    enc += [('lstm', i, c), ('elu', i + 1), ('conv', i + 2, c, cfg['hidden_size'], cfg['last_kernel_size'], 1)]
    dec, i = [('conv', 0, cfg['hidden_size'], c, cfg['kernel_size'], 1), ('lstm', 1, c)], 2
    for r in cfg['upsampling_ratios']:
        dec += [('elu', i), ('convtr', i + 1, c, c // 2, r)]
        i, c = i + 2, c // 2
        for j in range(cfg['num_residual_layers']):
            dec.append(('res', i, c, cfg['dilation_growth_rate'] ** j))
            i += 1
    dec += [('elu', i), ('conv', i + 1, c, 1, cfg['last_kernel_size'], 1)]
    return enc, dec


def _conv_prefixes(cfg):
    """prefix -> weight shape of every (transposed) conv, '<side>.layers.<i>[.block.<j> | .shortcut]'"""
    out = {}
    for side, lay in zip(('encoder', 'decoder'), _layout(cfg)):
        for e in lay:
            p = f'{side}.layers.{e[1]}'
            if e[0] == 'conv':
                out[p] = (e[3], e[2], e[4])
            elif e[0] == 'convtr':
                out[p] = (e[2], e[3], 2 * e[4])
            elif e[0] == 'res':
                hid = e[2] // cfg['compress']
                out[p + '.block.1'] = (hid, e[2], cfg['residual_kernel_size'])
                out[p + '.block.3'] = (e[2], hid, 1)
                if cfg['use_conv_shortcut']:
                    out[p + '.shortcut'] = (e[2], e[2], 1)
    return out


def _convtr_layers(upsampling_ratios, num_residual_layers):
    return {3 + i * (2 + num_residual_layers) for i in range(len(upsampling_ratios))}


def meta_to_hf_state_dict(state_dict):
    """`EncodecModel.state_dict()` of Meta's `encodec` package (encoder.model.N.conv.conv.weight_g, decoder.model.N.convtr.convtr.*,
    quantizer.vq.layers.Q._codebook.embed, ...) -> the same tensors under the transformers names this module loads.  KeyError on a key with no
    counterpart.  Written from the two packages' published module trees and round-trip tested only: never checked against a real Meta checkpoint."""
    out = {}
    for k, v in state_dict.items():
        n = re.sub(r'^(encoder|decoder)\.model\.', r'\1.layers.', k)
        n = re.sub(r'\.(conv\.conv|convtr\.convtr)\.', '.conv.', n)
        n = re.sub(r'^quantizer\.vq\.layers\.(\d+)\._codebook\.', r'quantizer.layers.\1.codebook.', n)
        if n == k or not re.match(r'^((encoder|decoder)\.layers\.\d+\.|quantizer\.layers\.\d+\.codebook\.)', n):
            raise KeyError(f'no counterpart for the key {k!r}')
        out[n] = v
    return out


def hf_to_meta_state_dict(state_dict, upsampling_ratios=(8, 5, 4, 2), num_residual_layers=1):
    """the inverse of meta_to_hf_state_dict; the geometry tells which decoder layers are transposed convs.  Same caveat: round-trip tested only."""
    tr = _convtr_layers(upsampling_ratios, num_residual_layers)
    out = {}
    for k, v in state_dict.items():
        m = re.match(r'^(encoder|decoder)\.layers\.(\d+)\.(.*)$', k)
        q = re.match(r'^quantizer\.layers\.(\d+)\.codebook\.(.*)$', k)
        if q:
            out[f'quantizer.vq.layers.{q.group(1)}._codebook.{q.group(2)}'] = v
        elif m:
            side, i, rest = m.group(1), int(m.group(2)), m.group(3)
            inner = 'convtr.convtr.' if side == 'decoder' and i in tr and rest.startswith('conv.') else 'conv.conv.'
            rest = re.sub(r'(^|\.)conv\.', lambda g: g.group(1) + inner, rest, count=1) if not rest.startswith('lstm.') else rest
            out[f'{side}.model.{i}.{rest}'] = v
        else:
            raise KeyError(f'no counterpart for the key {k!r}')
    return out


def _load_file(path):
    path = str(path)
    if not os.path.exists(path):
        raise FileNotFoundError(f'checkpoint_path {path} does not exist (a local file is required: hub names are never resolved)')
    try:
        sd = load_weights(path)
    except ImportError as e:
        raise NotImplementedError('.safetensors checkpoints need the `safetensors` package, which is not installed: pass a torch.load-able file') from e
    return sd['state_dict'] if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict) else sd


def lstm_image(weights, num_layers):
    """nn.LSTM's weight_ih_l{l} / weight_hh_l{l} / bias_ih_l{l} / bias_hh_l{l} (fp32, on the GPU) -> what lstm_skip reads: W_ih_l0 transposed as the
    activation operand [1, H, 4H] of the projection GEMM, the weights stacked [L, 4H, H], the two biases folded [L, 4H]"""
    L = num_layers
    return (weights['weight_ih_l0'].t().contiguous()[None],
            torch.stack([weights[f'weight_ih_l{l}'] for l in range(L)]).contiguous(),
            torch.stack([weights[f'weight_hh_l{l}'] for l in range(L)]).contiguous(),
            torch.stack([weights[f'bias_ih_l{l}'] + weights[f'bias_hh_l{l}'] for l in range(L)]).contiguous())


def lstm_skip(image, x):
    """x fp32 [B, H, T] -> lstm(x) + x, same layout (EncodecLSTM): layer 0's input projection for every step is ONE GEMM (alm_conv1d_valid, k = 1, with the
    steps as its output rows: xproj [T, B, 4H], a step's rows contiguous), the recurrence one launch per step from one call (alm_lstm_seq)"""
    wih0_t, w_ih, w_hh, bias = image
    B, H, T = x.shape
    xs = x.permute(2, 0, 1).contiguous()                            # [T, B, H]
    xproj = ops.conv1d_valid(wih0_t, xs.view(T * B, H, 1)).view(T, B, 4 * H)            # out[t b][g] = sum_k x[t b][k] W_ih[g][k]
    return ops.lstm_seq(xproj, w_ih, w_hh, bias, skip=xs, out_bct=True)


class EncodecWrapper(FrozenModel):
    """Positional order and members of the reference class (encodec.py:37-43).  `num_quantizers` is accepted and, as in the reference, replaced by what
    `bandwidth` selects.  Weights: keyword-only `checkpoint_path` (a torch.load-able state dict, or .safetensors where that package is installed) or
    `EncodecWrapper.from_state_dict`.  `config`: num_filters, upsampling_ratios, hidden_size, codebook_size, num_lstm_layers, kernel_size, last_kernel_size,
    residual_kernel_size, num_residual_layers, dilation_growth_rate, compress, use_conv_shortcut, sampling_rate (defaults: the 24 kHz model), and the
    options that raise when they leave the causal weight-norm mono model."""

    def __init__(self, target_sample_hz=24000, strides=(2, 4, 5, 8), num_quantizers=8, bandwidth=6.0, *, checkpoint_path=None, **config):
        super().__init__()
        if checkpoint_path is None:
            raise NotImplementedError('EncodecWrapper needs local weights: pass checkpoint_path=<file> or use EncodecWrapper.from_state_dict(state_dict). '
                                      'Hub names are never resolved and nothing is downloaded (the reference calls EncodecModel.encodec_model_24khz())')
        self._setup(_load_file(checkpoint_path), target_sample_hz, strides, bandwidth, config)

    @classmethod
    def from_state_dict(cls, state_dict, target_sample_hz=24000, strides=(2, 4, 5, 8), bandwidth=6.0, **config):
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._setup(state_dict, target_sample_hz, strides, bandwidth, dict(config))
        return self

    def _setup(self, state_dict, target_sample_hz, strides, bandwidth, config):
        unknown = set(config) - set(_CONFIG) - set(_UNSUPPORTED)
        if unknown:
            raise TypeError(f'unknown configuration keys {sorted(unknown)}')
        for key, only in _UNSUPPORTED.items():
            if key in config and config[key] != only:
                raise NotImplementedError(f'{key}={config[key]!r} is not implemented: only the causal weight-norm mono 24 kHz model ({key}={only!r})')
        cfg = dict(_CONFIG, **{k: v for k, v in config.items() if k in _CONFIG})
        cfg['upsampling_ratios'] = tuple(int(r) for r in cfg['upsampling_ratios'])
        if cfg['num_lstm_layers'] not in (1, 2):
            raise NotImplementedError(f"num_lstm_layers={cfg['num_lstm_layers']} is not implemented (1 or 2)")
        self.config = cfg
        self.target_sample_hz = target_sample_hz
        assert self.target_sample_hz == 24000, "haven't done anything with non-24kHz yet"
        self.strides = tuple(strides)
        if self.seq_len_multiple_of != math.prod(cfg['upsampling_ratios']):
            raise ValueError(f"strides {self.strides} do not multiply to the model's hop {math.prod(cfg['upsampling_ratios'])}")
        self.codebook_dim = cfg['hidden_size']
        self.codebook_size = cfg['codebook_size']
        self.rq_groups = 1
        self.bandwidth = float(bandwidth)
        frame_rate = math.ceil(cfg['sampling_rate'] / math.prod(cfg['upsampling_ratios']))
        self.num_quantizers = int(max(1, math.floor(self.bandwidth * 1000 / (math.log2(cfg['codebook_size']) * frame_rate))))

        sd = {}
        for k, v in state_dict.items():
            k = k.replace('.parametrizations.weight.original0', '.weight_g').replace('.parametrizations.weight.original1', '.weight_v')
            if not _IGNORED.match(k):
                sd[k] = v
        names, shapes = [], {}
        for p, shape in _conv_prefixes(cfg).items():
            names += [p + '.conv.weight_g', p + '.conv.weight_v', p + '.conv.bias']
            shapes[p + '.conv.weight_v'] = shape
        for side, lay in zip(('encoder', 'decoder'), _layout(cfg)):
            for e in lay:
                if e[0] == 'lstm':
                    for l in range(cfg['num_lstm_layers']):
                        names += [f'{side}.layers.{e[1]}.lstm.{n}_l{l}' for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
                        shapes[f'{side}.layers.{e[1]}.lstm.weight_ih_l{l}'] = shapes[f'{side}.layers.{e[1]}.lstm.weight_hh_l{l}'] = (4 * e[2], e[2])
        books = sorted(int(k.split('.')[2]) for k in sd if re.match(r'^quantizer\.layers\.\d+\.codebook\.embed$', k))
        if books != list(range(len(books))) or len(books) < self.num_quantizers:
            raise KeyError(f'bandwidth {self.bandwidth} needs codebooks 0 .. {self.num_quantizers - 1}; the state dict holds {books}')
        self._adopt(names, sd, 'the EnCodec model', lambda k: k.startswith('quantizer.layers.'))
        for n, shape in shapes.items():
            if tuple(sd[n].shape) != shape:
                raise ValueError(f'{n}: shape {tuple(sd[n].shape)} does not match the configuration ({shape})')
        for q in books:
            E = sd[f'quantizer.layers.{q}.codebook.embed']
            if tuple(E.shape) != (cfg['codebook_size'], cfg['hidden_size']):
                raise ValueError(f"codebook {q}: shape {tuple(E.shape)} does not match ({cfg['codebook_size']}, {cfg['hidden_size']})")
            self._slot(f'quantizer.layers.{q}.codebook.embed').register_buffer('embed', E.detach().to(F32).clone().contiguous())
        self.num_codebooks = len(books)
        self.eval()

    # ---- derived tensors, computed once per load / device move ------------------------------------------------------------------------------------

    def _prepare(self):
        """weight norm folded (w = g v / |v|, the norm over every axis but 0 -- for the transposed conv's [Cin, Cout, k] weight axis 0 is the INPUT
        channel, torch.nn.utils.weight_norm's default dim), the MFMA images of the conv weights and of the codebooks, the LSTM weights stacked"""
        if 'images' in self._cache:
            return self._cache['images']
        cfg, t = self.config, self._params()
        im = {}
        tr = {f'decoder.layers.{e[1]}': e for e in _layout(cfg)[1] if e[0] == 'convtr'}
        for p in _conv_prefixes(cfg):
            g, v, b = t[p + '.conv.weight_g'], t[p + '.conv.weight_v'], t[p + '.conv.bias']
            w = (g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)).contiguous()
            if p in tr:                                             # k = 2 zero-padded conv over phase-major channels (soundstream.CausalConvTranspose1d)
                s, (cin, cout, _) = tr[p][4], w.shape
                w2 = torch.stack((w[:, :, s:], w[:, :, :s]), dim=-1).permute(2, 1, 0, 3).reshape(s * cout, cin, 2).contiguous()
                im[p] = (ops.conv1d_pack(w2), b.repeat(s).contiguous(), cout, s)
            else:
                im[p] = (ops.conv1d_pack(w), b, w.shape[0], w.shape[2])
        for side, lay in zip(('encoder', 'decoder'), _layout(cfg)):
            for e in lay:
                if e[0] == 'lstm':
                    p = f'{side}.layers.{e[1]}.lstm'
                    im[p] = lstm_image({k[len(p) + 1:]: v for k, v in t.items() if k.startswith(p + '.')}, cfg['num_lstm_layers'])
        b = dict(self.named_buffers())
        E = torch.stack([b[f'quantizer.layers.{q}.codebook.embed'] for q in range(self.num_codebooks)]).contiguous()
        im['codebooks'] = (E, E[:self.num_quantizers].contiguous()) + ops.rvq_pack(E[:self.num_quantizers].contiguous())
        self._cache['images'] = im
        return im

    # ---- the layers -----------------------------------------------------------------------------------------------------------------------------

    def _conv(self, p, x, *, stride=1, dilation=1, pre_elu=False, elu=False, residual=None):
        wp, bias, cout, k = self._prepare()[p]
        T = x.shape[-1]
        left, right = dilation * (k - 1) + 1 - stride, -T % stride
        if T <= max(left, right):
            raise ValueError(f'{T} steps are too few for the reflect padding of {p} ({max(left, right)}): EncodecWrapper needs at least '
                             f"{self.config['last_kernel_size']} frames ({self.config['last_kernel_size'] * self.downsample_factor} samples)")
        if right:           # a ragged length: each strided conv reflect-pads its input on the right up to the next multiple of its stride
            x = F.pad(x, (0, right), mode='reflect')
        return ops.conv1d_causal_pre(x, wp, bias, cout, k, stride=stride, dilation=dilation, pre_elu=pre_elu, elu=elu, residual=residual)

    def _convtr(self, p, x, pre_elu):
        wp, bias, cout, s = self._prepare()[p]
        y = ops.conv1d_causal_pre(x, wp, bias, s * cout, 2, pre_elu=pre_elu, zero_pad=True)
        return ops.phase_interleave(y, cout, s)

    def _run(self, side, lay, x):
        pre = False
        for e in lay:
            p = f'{side}.layers.{e[1]}'
            if e[0] == 'elu':
                pre = True
                continue
            if e[0] == 'conv':
                x = self._conv(p, x, stride=e[5], pre_elu=pre)
            elif e[0] == 'convtr':
                x = self._convtr(p, x, pre)
            elif e[0] == 'lstm':
                x = lstm_skip(self._prepare()[p + '.lstm'], x)
            else:           # shortcut(x) + conv_1x1(ELU(conv_k3(ELU(x)))): the k3 conv stores its output through the ELU, the 1x1 conv adds the shortcut
                sc = self._conv(p + '.shortcut', x) if self.config['use_conv_shortcut'] else x
                h = self._conv(p + '.block.1', x, dilation=e[3], pre_elu=True, elu=True)
                x = self._conv(p + '.block.3', h, residual=sc)
            pre = False
        return x

    def _check(self, x):
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.EncodecWrapper runs on the MI355X only (no CPU fallback)')

    # ---- the reference's members ----------------------------------------------------------------------------------------------------------------

    @property
    def seq_len_multiple_of(self):
        return functools.reduce(lambda x, y: x * y, self.strides)

    @property
    def downsample_factor(self):
        return self.seq_len_multiple_of

    @torch.no_grad()
    def encode(self, wave):
        """wave (b, t) at 24 kHz -> encoder output fp32 (b, ceil(t / 320), 128)"""
        self._check(wave)
        if wave.dim() != 2:
            raise ValueError(f'wave must be (batch, samples), got {tuple(wave.shape)}')
        least = self.config['last_kernel_size'] * self.downsample_factor
        if wave.shape[1] < least:       # the last conv reflects kernel_size - 1 frames; transformers zero-extends a shorter input first, which is not implemented
            raise ValueError(f'{wave.shape[1]} samples are fewer than {least} ({self.config["last_kernel_size"]} frames): too short for EncodecWrapper')
        return ops.bct_to_btc(self._run('encoder', _layout(self.config)[0], wave.to(F32).unsqueeze(1).contiguous()))

    @torch.no_grad()
    def quantize(self, feats):
        """fp32 (b, n, d) -> codes int64 (b, n, num_quantizers): nearest code per level, the first index on ties"""
        b, n, d = feats.shape
        _, E, Et, e2 = self._prepare()['codebooks']
        return ops.rvq_encode(feats.reshape(b * n, d), E, Et, e2).view(b, n, self.num_quantizers)

    @torch.no_grad()
    def forward(self, x, input_sample_hz=None, return_encoded=False, **kwargs):       # encodec.py:94-136
        self._check(x)
        lead = x.shape[:-1]
        x = x.reshape(-1, x.shape[-1])                              # pack([x], '* n')
        if input_sample_hz is not None:
            x = resample(x, input_sample_hz, self.target_sample_hz)
        codes = self.quantize(self.encode(x))
        emb = None
        if return_encoded:
            emb = self.get_emb_from_indices(codes)
            emb = emb.reshape(*lead, *emb.shape[1:])
        return emb, codes.reshape(*lead, *codes.shape[1:]), None

    @torch.no_grad()
    def get_emb_from_indices(self, indices):                        # encodec.py:157-160
        """codes int (b, n, q) -> the sum of the code vectors fp32 (b, n, 128)"""
        self._check(indices)
        b, n, q = indices.shape
        E = self._prepare()['codebooks'][0]
        if q > E.shape[0]:
            raise ValueError(f'{q} quantizer levels, the model has {E.shape[0]} codebooks')
        out = torch.empty((b * n, self.codebook_dim), dtype=F32, device=indices.device)
        ops.rvq_decode(indices.to(torch.int64).reshape(b * n, q).contiguous(), E[:q].contiguous(), out)
        return out.view(b, n, self.codebook_dim)

    @torch.no_grad()
    def decode(self, emb):                                          # encodec.py:162-164
        """fp32 (b, n, 128) -> wave (b, 1, n * 320)"""
        self._check(emb)
        return self._run('decoder', _layout(self.config)[1], ops.bct_to_btc(emb.to(F32).contiguous()))

    @torch.no_grad()
    def decode_from_codebook_indices(self, quantized_indices):      # encodec.py:138-155
        """codes (b, n, q) -> wave (b, 1, n * 320), every batch row decoded on its own (the reference overlap-adds the rows of a batch as if they were
        frames of one clip)"""
        return self.decode(self.get_emb_from_indices(quantized_indices))
