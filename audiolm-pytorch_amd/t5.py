"""The T5 text encoder on the MI355X: token ids -> zero-masked text embeddings (reference t5.py:68-110) without Hugging Face on the hot path.

The reference runs `transformers.T5EncoderModel` in eager torch inside every conditioned training step.  Here the encoder (T5Stack: shared embedding,
pre-norm blocks of relative-position-biased self-attention and a (gated) feed-forward, final norm) is restated on the project's fp32 kernels
(csrc/t5.hip; alm_conv1d_valid and the attention: csrc/dense_f32.hip), activations [C][B * T]:

  ids [B, T] -> shared[ids]                                                                  alm_t5_embed
             -> L blocks: x += o(attn(q | k | v (norm(x)), bias, mask)); x += wo(gate(wi (norm(x))))   alm_t5_rmsnorm, alm_conv1d_valid (k = 1),
                                                                                             alm_t5_attn_fwd, alm_t5_gate
             -> final norm, zeros where the mask is 0, written as (b, n, d_model)            alm_t5_rmsnorm (transposed form)

Parameters are registered under transformers' `T5EncoderModel` key names, so such a state dict loads by name.  Weights come from local files only:
nothing here resolves a hub name or opens a connection.  A model is made known to `t5_encode_text` / the transformers' `text=` argument by
`register_t5(name, encoder, tokenizer)` or `load_t5(name, directory)`; a name that was never registered raises NotImplementedError.
"""
from __future__ import annotations

import json
import math
import os
import re

import torch

from . import ops
from .frozen import FrozenModel, load_weights

MAX_LENGTH = 256
DEFAULT_T5_NAME = 'google/t5-v1_1-base'

# d_model of the published checkpoints: sizes proj_text_embed of a conditioned transformer whose T5 was not registered (pre-computed text_embeds)
_T5_DIMS = {'google/t5-v1_1-small': 512, 'google/t5-v1_1-base': 768, 'google/t5-v1_1-large': 1024,
            'google/t5-v1_1-xl': 2048, 'google/t5-v1_1-xxl': 4096, 't5-small': 512, 't5-base': 768, 't5-large': 1024}

_IGNORED = re.compile(r'^(decoder\.|lm_head\.)')
_ALIAS = 'encoder.embed_tokens.weight'
_BIAS_KEY = 'encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight'


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """transformers T5Attention._relative_position_bucket(bidirectional=True), the same fp32 torch expression term by term: the bucket boundaries
    at |delta| = 8 * 16 ** (k / 8) are integers in real arithmetic, so which side they fall on is decided by this expression's fp32 rounding.
    relative_position: int64 tensor of key - query -> int64 bucket indices in [0, num_buckets)."""
    relative_position = relative_position.to(torch.long)
    num_buckets //= 2
    relative_buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    relative_position_if_large = max_exact + (
        torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    relative_position_if_large = torch.min(relative_position_if_large, torch.full_like(relative_position_if_large, num_buckets - 1))
    return relative_buckets + torch.where(is_small, relative_position, relative_position_if_large)


class T5Encoder(FrozenModel):
    """`transformers.T5EncoderModel`, frozen, fp32, GPU only.  Build it with from_state_dict / from_pretrained."""

    def __init__(self, state_dict, *, num_heads, d_kv=64, feed_forward_proj='gated-gelu', relative_attention_num_buckets=32,
                 relative_attention_max_distance=128, layer_norm_epsilon=1e-6, is_decoder=False):
        super().__init__()
        if is_decoder:
            raise NotImplementedError('is_decoder=True: only the T5 encoder is implemented (no causal mask, no cross-attention)')
        if int(d_kv) != 64:
            raise NotImplementedError(f'd_kv={d_kv} is not implemented: the attention kernel handles heads of width 64 only')
        if feed_forward_proj not in ('gated-gelu', 'relu'):
            raise NotImplementedError(f"feed_forward_proj={feed_forward_proj!r} is not implemented: 'gated-gelu' (the v1.1 models) or 'relu' (the "
                                      'original t5-small / base / large)')
        self.num_heads, self.d_kv, self.gated = int(num_heads), 64, feed_forward_proj == 'gated-gelu'
        self.feed_forward_proj = feed_forward_proj
        self.num_buckets, self.max_distance = int(relative_attention_num_buckets), int(relative_attention_max_distance)
        self.eps = float(layer_norm_epsilon)

        sd = state_dict
        if _ALIAS in sd and 'shared.weight' not in sd:
            sd = {**sd, 'shared.weight': sd[_ALIAS]}
        layers = {int(m.group(1)) for m in (re.match(r'encoder\.block\.(\d+)\.', k) for k in sd) if m}
        self.num_layers = L = max(layers) + 1 if layers else 0
        ff = ('wi_0', 'wi_1', 'wo') if self.gated else ('wi', 'wo')
        names = ['shared.weight', _BIAS_KEY, 'encoder.final_layer_norm.weight']
        for i in range(L):
            names += [f'encoder.block.{i}.layer.0.SelfAttention.{n}.weight' for n in 'qkvo']
            names += [f'encoder.block.{i}.layer.{j}.layer_norm.weight' for j in (0, 1)]
            names += [f'encoder.block.{i}.layer.1.DenseReluDense.{n}.weight' for n in ff]
        what = f'a {L}-block {feed_forward_proj} T5 encoder'
        if L == 0:
            raise self._lacks([n for n in names if n not in sd], what)
        self._adopt(names, sd, what, lambda k: _IGNORED.match(k) or k == _ALIAS)

        p = self._params()
        self.vocab_size, self.d_model = p['shared.weight'].shape
        inner = self.num_heads * 64
        if tuple(p[_BIAS_KEY].shape) != (self.num_buckets, self.num_heads):
            raise ValueError(f'relative_attention_bias is {tuple(p[_BIAS_KEY].shape)}, expected ({self.num_buckets}, {self.num_heads}) = '
                             '(relative_attention_num_buckets, num_heads)')
        self.d_ff = p[f'encoder.block.0.layer.1.DenseReluDense.{ff[0]}.weight'].shape[0]
        for i in range(L):
            pre = f'encoder.block.{i}.layer.'
            want = {**{f'0.SelfAttention.{n}.weight': (inner, self.d_model) for n in 'qkv'}, '0.SelfAttention.o.weight': (self.d_model, inner),
                    '0.layer_norm.weight': (self.d_model,), '1.layer_norm.weight': (self.d_model,),
                    **{f'1.DenseReluDense.{n}.weight': (self.d_ff, self.d_model) for n in ff[:-1]}, '1.DenseReluDense.wo.weight': (self.d_model, self.d_ff)}
            for k, shape in want.items():
                if tuple(p[pre + k].shape) != shape:
                    raise ValueError(f'{pre + k} is {tuple(p[pre + k].shape)}, expected {shape} ({self.num_heads} heads of 64)')
        self._fold()
        self.eval()

    @classmethod
    def from_state_dict(cls, state_dict, *, num_heads, d_kv=64, feed_forward_proj='gated-gelu', relative_attention_num_buckets=32,
                        relative_attention_max_distance=128, layer_norm_epsilon=1e-6, **config):
        """builds the encoder from a `T5EncoderModel` (or full `T5ForConditionalGeneration`: decoder.* and lm_head.* are ignored) state dict.
        `config` takes is_decoder (raises when set) and nothing else."""
        if set(config) - {'is_decoder'}:
            raise TypeError(f'unknown configuration keys {sorted(set(config) - {"is_decoder"})}')
        return cls(state_dict, num_heads=num_heads, d_kv=d_kv, feed_forward_proj=feed_forward_proj,
                   relative_attention_num_buckets=relative_attention_num_buckets, relative_attention_max_distance=relative_attention_max_distance,
                   layer_norm_epsilon=layer_norm_epsilon, **config)

    @classmethod
    def from_pretrained(cls, directory):
        """a LOCAL directory holding config.json and model.safetensors or pytorch_model.bin (what `save_pretrained` writes).  A string that is not
        an existing directory raises FileNotFoundError: hub names are never resolved."""
        directory = os.fspath(directory)
        if not os.path.isdir(directory):
            raise FileNotFoundError(f'{directory!r} is not a directory: T5Encoder.from_pretrained reads local files only (config.json + '
                                    'model.safetensors / pytorch_model.bin) and never resolves a hub name')
        with open(os.path.join(directory, 'config.json')) as fh:
            cfg = json.load(fh)
        files = [f for f in (os.path.join(directory, n) for n in ('model.safetensors', 'pytorch_model.bin')) if os.path.exists(f)]
        if not files:
            raise FileNotFoundError(f'{directory!r} holds neither model.safetensors nor pytorch_model.bin')
        sd = load_weights(files[0])
        ffp = cfg.get('feed_forward_proj', 'relu')
        return cls(sd, num_heads=cfg['num_heads'], d_kv=cfg.get('d_kv', 64), feed_forward_proj=ffp,
                   relative_attention_num_buckets=cfg.get('relative_attention_num_buckets', 32),
                   relative_attention_max_distance=cfg.get('relative_attention_max_distance', 128),
                   layer_norm_epsilon=cfg.get('layer_norm_epsilon', 1e-6), is_decoder=bool(cfg.get('is_decoder', False)))

    def _fold(self):
        """derived tensors, computed at load and after load_state_dict: q | k | v and wi_0 | wi_1 stacked for one launch each, every Linear weight
        in the [Cout, Cin, 1] form of alm_conv1d_valid; the per-length bias tables are rebuilt on demand"""
        p = self._params()
        for i in range(self.num_layers):
            att, ffn = f'encoder.block.{i}.layer.0.SelfAttention.', f'encoder.block.{i}.layer.1.DenseReluDense.'
            self.register_buffer(f'_qkv_w{i}', torch.cat([p[att + f'{n}.weight'] for n in 'qkv']).unsqueeze(-1).contiguous(), persistent=False)
            wi = torch.cat([p[ffn + 'wi_0.weight'], p[ffn + 'wi_1.weight']]) if self.gated else p[ffn + 'wi.weight']
            self.register_buffer(f'_wi_w{i}', wi.unsqueeze(-1).contiguous(), persistent=False)

    def bias_table(self, T, device=None):
        """fp32 [H, 2 T - 1]: entry [h][j - i + T - 1] = relative_attention_bias[bucket(j - i)][h], the whole of T5's position bias for sequences of
        T tokens (it depends on (h, j - i) only).  Built once per (T, device) and kept."""
        w = self.get_parameter(_BIAS_KEY)
        device = w.device if device is None else torch.device(device)

        def build():
            bucket = relative_position_bucket(torch.arange(-(T - 1), T, dtype=torch.long), self.num_buckets, self.max_distance)
            return w.detach().to(device)[bucket.to(device)].t().contiguous()
        return self._cached(('bias_table', int(T), device.type, device.index), build)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None):
        """input_ids integer (b, n), attention_mask (b, n) of 0 / 1 or None (all valid) -> fp32 (b, n, d_model), exact zeros where the mask is 0"""
        if not input_ids.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.T5Encoder runs on the MI355X only (no CPU fallback)')
        if input_ids.dim() != 2 or input_ids.is_floating_point():
            raise ValueError(f'input_ids must be integer (batch, tokens), got {input_ids.dtype} {tuple(input_ids.shape)}')
        B, T = input_ids.shape
        if B == 0 or T == 0:
            raise ValueError(f'empty input_ids {tuple(input_ids.shape)}')
        device = input_ids.device
        mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, T):
                raise ValueError(f'attention_mask {tuple(attention_mask.shape)} does not match input_ids {(B, T)}')
            mask = (attention_mask.to(device) != 0).to(torch.uint8).contiguous()
        p, w1 = self._params(), self._linear
        bias = self.bias_table(T, device)
        lin = lambda t, w, res=None: ops.conv1d_valid(t.unsqueeze(0), w, residual=None if res is None else res.unsqueeze(0))[0]      # noqa: E731
        x = ops.t5_embed(input_ids.to(torch.long).contiguous(), p['shared.weight'])
        for i in range(self.num_layers):
            pre = f'encoder.block.{i}.layer.'
            h = ops.t5_rmsnorm(x, p[pre + '0.layer_norm.weight'], self.eps)
            a = ops.t5_attn(lin(h, getattr(self, f'_qkv_w{i}')), bias, mask, B, self.num_heads)
            x = lin(a, w1(pre + '0.SelfAttention.o.weight'), x)
            h = ops.t5_rmsnorm(x, p[pre + '1.layer_norm.weight'], self.eps)
            g = ops.t5_gate(lin(h, getattr(self, f'_wi_w{i}')), self.gated)
            x = lin(g, w1(pre + '1.DenseReluDense.wo.weight'), x)
        out = ops.t5_rmsnorm(x, p['encoder.final_layer_norm.weight'], self.eps, mask=None if mask is None else mask.view(-1), transpose_out=True)
        return out.view(B, T, self.d_model)


# ---- the registry behind t5_encode_text and the transformers' `text=` ----
_REGISTRY = {}


def register_t5(name, encoder, tokenizer):
    """makes `name` (a transformer's t5_name) resolve to `encoder` (a T5Encoder) and `tokenizer`: any callable with the Hugging Face call form
    tokenizer(texts, return_tensors='pt', padding='longest', max_length=..., truncation=True) -> object with .input_ids and .attention_mask"""
    if not isinstance(encoder, T5Encoder):
        raise TypeError(f'encoder must be an audiolm_pytorch_amd.T5Encoder, got {type(encoder).__name__}')
    if not callable(tokenizer):
        raise TypeError('tokenizer must be callable')
    _REGISTRY[name] = (encoder, tokenizer)
    return encoder


def unregister_t5(name):
    _REGISTRY.pop(name, None)


def load_t5(name, directory, tokenizer=None):
    """register_t5(name, T5Encoder.from_pretrained(directory), tokenizer); tokenizer=None: transformers.T5Tokenizer from the same local directory"""
    encoder = T5Encoder.from_pretrained(directory)
    if tokenizer is None:
        try:
            from transformers import T5Tokenizer
        except ImportError as e:
            raise ImportError('load_t5(tokenizer=None) takes the tokenizer from `transformers`, which is not installed: pass tokenizer=<callable> '
                              '(texts, return_tensors, padding, max_length, truncation) -> .input_ids, .attention_mask') from e
        tokenizer = T5Tokenizer.from_pretrained(os.fspath(directory), local_files_only=True)
    if torch.cuda.is_available():
        encoder = encoder.cuda()
    return register_t5(name, encoder, tokenizer)


def get_encoded_dim(name):
    """d_model of the text encoder `name` (reference t5.py:get_encoded_dim): a registered encoder's own width, else the published checkpoints' widths"""
    if name in _REGISTRY:
        return _REGISTRY[name][0].d_model
    return _T5_DIMS.get(name, 768)


def t5_encode_text(texts, name=DEFAULT_T5_NAME, output_device=None):
    """reference t5.py:68-110: texts (str or list of str) -> fp32 (b, n, d_model), zeros at the padded positions"""
    if isinstance(texts, str):
        texts = [texts]
    if name not in _REGISTRY:
        raise NotImplementedError(f'no T5 text encoder is registered under {name!r} (hub names are never resolved): register a local one with '
                                  'audiolm_pytorch_amd.load_t5(name, directory) / register_t5(name, encoder, tokenizer), or pass pre-computed '
                                  '`text_embeds` (b, m, cond_dim) instead of `text`')
    encoder, tokenizer = _REGISTRY[name]
    encoded = tokenizer(texts, return_tensors='pt', padding='longest', max_length=MAX_LENGTH, truncation=True)
    device = encoder.get_parameter('shared.weight').device
    out = encoder(encoded.input_ids.to(device), encoded.attention_mask.to(device))
    return out if output_device is None else out.to(output_device)
