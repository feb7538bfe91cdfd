"""HubertWithKmeans on the MI355X: raw wave -> semantic token ids (reference hubert_kmeans.py:37-121) without fairseq.

The reference runs a fairseq HuBERT-base feature model (`model(wav, features_only=True, mask=False, output_layer=L)['x']`) and assigns each 20 ms
frame to its nearest k-means centre (`(-cdist(embed, centres)).argmax(-1)`).  Here the model is restated on the project's fp32 kernels
(csrc/hubert.hip, csrc/dense_f32.hip, csrc/codec.hip), in the codec's [B][C][T] layout:

  wave [B, T] -> conv0 (1 -> C, k 10, stride 5) + GroupNorm(C, C) over time + GELU     alm_hubert_conv0_stats / _apply
              -> 6 bias-less convs (k 3 3 3 3 2 2, stride 2) + GELU                       alm_conv1d_valid
              -> LayerNorm(C) -> Linear(C, D)                                             alm_layernorm_bct_split, alm_conv1d_valid (k = 1)
              -> x + GELU(pos_conv(x)) (weight-normed, k 128, pad 64, 16 groups, last sample dropped) -> LayerNorm(D)
              -> L post-LN layers: x = LN(x + out(attn(q, k, v))); x = LN(x + fc2(GELU(fc1(x))))   alm_mha_attn_fwd + the above
              -> 'b d n -> b n d' -> nearest centre                                       alm_bct_to_btc, alm_rvq_encode (one quantizer)

Parameters are registered under fairseq's key names, so the 'model' dict of a fairseq HuBERT-base checkpoint loads by name.  Everything outside the
documented architecture raises NotImplementedError; a CPU tensor raises RuntimeError (there is no CPU path).
"""
from __future__ import annotations

import ast
import os
import pickle
import re

import torch
from torch import nn

from . import ops
from .frozen import F32, FrozenModel, load_weights
from .resample import resample
from .soundstream import curtail_to_multiple

BASE_CONV_LAYERS = '[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2'
_IGNORED = re.compile(r'^(mask_emb$|final_proj\.|label_embs_concat$|target_glu\.)')
_LAYER_KEYS = [f'{m}.{p}' for m in ('self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj', 'self_attn.out_proj', 'self_attn_layer_norm', 'fc1', 'fc2',
                                    'final_layer_norm') for p in ('weight', 'bias')]

_HF_RULES = [   # (Hugging Face HubertModel name, fairseq name), regex with one layer index where needed
    (r'feature_extractor\.conv_layers\.(\d+)\.conv\.weight', r'feature_extractor.conv_layers.\1.0.weight'),
    (r'feature_extractor\.conv_layers\.0\.layer_norm\.(weight|bias)', r'feature_extractor.conv_layers.0.2.\1'),
    (r'feature_projection\.layer_norm\.(weight|bias)', r'layer_norm.\1'),
    (r'feature_projection\.projection\.(weight|bias)', r'post_extract_proj.\1'),
    (r'encoder\.pos_conv_embed\.conv\.bias', r'encoder.pos_conv.0.bias'),
    (r'encoder\.pos_conv_embed\.conv\.(?:weight_g|parametrizations\.weight\.original0)', r'encoder.pos_conv.0.weight_g'),
    (r'encoder\.pos_conv_embed\.conv\.(?:weight_v|parametrizations\.weight\.original1)', r'encoder.pos_conv.0.weight_v'),
    (r'encoder\.layer_norm\.(weight|bias)', r'encoder.layer_norm.\1'),
    (r'encoder\.layers\.(\d+)\.attention\.(q|k|v|out)_proj\.(weight|bias)', r'encoder.layers.\1.self_attn.\2_proj.\3'),
    (r'encoder\.layers\.(\d+)\.layer_norm\.(weight|bias)', r'encoder.layers.\1.self_attn_layer_norm.\2'),
    (r'encoder\.layers\.(\d+)\.feed_forward\.intermediate_dense\.(weight|bias)', r'encoder.layers.\1.fc1.\2'),
    (r'encoder\.layers\.(\d+)\.feed_forward\.output_dense\.(weight|bias)', r'encoder.layers.\1.fc2.\2'),
    (r'encoder\.layers\.(\d+)\.final_layer_norm\.(weight|bias)', r'encoder.layers.\1.final_layer_norm.\2'),
    (r'masked_spec_embed', r'mask_emb'),
]
_FS_RULES = [
    (r'feature_extractor\.conv_layers\.(\d+)\.0\.weight', r'feature_extractor.conv_layers.\1.conv.weight'),
    (r'feature_extractor\.conv_layers\.0\.2\.(weight|bias)', r'feature_extractor.conv_layers.0.layer_norm.\1'),
    (r'layer_norm\.(weight|bias)', r'feature_projection.layer_norm.\1'),
    (r'post_extract_proj\.(weight|bias)', r'feature_projection.projection.\1'),
    (r'encoder\.pos_conv\.0\.bias', r'encoder.pos_conv_embed.conv.bias'),
    (r'encoder\.pos_conv\.0\.weight_g', r'encoder.pos_conv_embed.conv.weight_g'),
    (r'encoder\.pos_conv\.0\.weight_v', r'encoder.pos_conv_embed.conv.weight_v'),
    (r'encoder\.layer_norm\.(weight|bias)', r'encoder.layer_norm.\1'),
    (r'encoder\.layers\.(\d+)\.self_attn\.(q|k|v|out)_proj\.(weight|bias)', r'encoder.layers.\1.attention.\2_proj.\3'),
    (r'encoder\.layers\.(\d+)\.self_attn_layer_norm\.(weight|bias)', r'encoder.layers.\1.layer_norm.\2'),
    (r'encoder\.layers\.(\d+)\.fc1\.(weight|bias)', r'encoder.layers.\1.feed_forward.intermediate_dense.\2'),
    (r'encoder\.layers\.(\d+)\.fc2\.(weight|bias)', r'encoder.layers.\1.feed_forward.output_dense.\2'),
    (r'encoder\.layers\.(\d+)\.final_layer_norm\.(weight|bias)', r'encoder.layers.\1.final_layer_norm.\2'),
    (r'mask_emb', r'masked_spec_embed'),
]


def _rename(state_dict, rules, strip):
    out = {}
    for k, v in state_dict.items():
        name = k[len(strip):] if strip and k.startswith(strip) else k
        for pat, rep in rules:
            if re.fullmatch(pat, name):
                out[re.sub(pat, rep, name)] = v
                break
        else:
            raise KeyError(f'no counterpart for the key {k!r}')
    return out


def hf_to_fairseq_state_dict(state_dict):
    """Hugging Face `HubertModel.state_dict()` (a leading 'hubert.' is dropped; either spelling of the positional conv's weight norm) -> the same
    tensors under fairseq's key names, ready for `HubertWithKmeans.from_state_dict`.  KeyError on a key with no fairseq counterpart."""
    return _rename(state_dict, _HF_RULES, 'hubert.')


def fairseq_to_hf_state_dict(state_dict):
    """the inverse of hf_to_fairseq_state_dict (weight norm in the weight_g / weight_v spelling)"""
    return _rename(state_dict, _FS_RULES, None)


def _conv_spec(spec):
    """fairseq's conv_feature_layers: a list of (dim, kernel, stride) or the string fairseq evaluates ('[(512,10,5)] + [(512,3,2)] * 4 + ...');
    the string is parsed as lists / tuples / integers joined by + and *, nothing else."""
    if not isinstance(spec, str):
        return [tuple(int(v) for v in layer) for layer in spec]

    def ev(node):
        if isinstance(node, ast.Expression):
            return ev(node.body)
        if isinstance(node, ast.Constant) and isinstance(node.value, int):
            return node.value
        if isinstance(node, (ast.List, ast.Tuple)):
            vals = [ev(e) for e in node.elts]
            return vals if isinstance(node, ast.List) else tuple(vals)
        if isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Mult)):
            l, r = ev(node.left), ev(node.right)
            return l + r if isinstance(node.op, ast.Add) else l * r
        raise ValueError(f'conv_feature_layers: unsupported expression {spec!r}')
    return [tuple(int(v) for v in layer) for layer in ev(ast.parse(spec, mode='eval'))]


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    if hasattr(cfg, 'get'):
        v = cfg.get(key, default)
    else:
        v = getattr(cfg, key, default)
    return default if v is None else v


def frame_count(num_samples, conv_layers=None):
    """frames the feature extractor gives for `num_samples` samples: (T - 400) // 320 + 1 for the base conv stack"""
    n = int(num_samples)
    for _, k, s in _conv_spec(conv_layers or BASE_CONV_LAYERS):
        n = (n - k) // s + 1 if n >= k else 0
    return n


class HubertWithKmeans(FrozenModel):
    """Positional order, defaults and members of the reference class (hubert_kmeans.py:43-95).  `checkpoint_path`: torch.load-able, either a fairseq
    checkpoint ({'model': state dict, 'cfg': {'model': ..., 'task': ...}} or {'model': ..., 'args': Namespace}) or a bare state dict;
    `kmeans_path`: joblib file of an object with `cluster_centers_`, or a .pt / .npy file holding the (clusters, dim) array."""

    def __init__(self, checkpoint_path, kmeans_path, target_sample_hz=16000, seq_len_multiple_of=None, output_layer=9):
        super().__init__()
        assert os.path.exists(str(checkpoint_path)), f'path {checkpoint_path} does not exist'
        assert os.path.exists(str(kmeans_path)), f'path {kmeans_path} does not exist'
        try:
            ckpt = torch.load(str(checkpoint_path), map_location='cpu', weights_only=True)
        except pickle.UnpicklingError:              # fairseq checkpoints carry an argparse / omegaconf configuration object
            ckpt = torch.load(str(checkpoint_path), map_location='cpu', weights_only=False)
        config = {}
        if isinstance(ckpt, dict) and 'model' in ckpt and isinstance(ckpt['model'], dict):
            state_dict = ckpt['model']
            cfg = ckpt.get('cfg')
            model_cfg = _cfg_get(cfg, 'model') if cfg is not None else ckpt.get('args')
            task_cfg = _cfg_get(cfg, 'task') if cfg is not None else ckpt.get('args')
            for key in ('conv_feature_layers', 'encoder_attention_heads', 'conv_pos', 'conv_pos_groups', 'layer_norm_first', 'extractor_mode', 'conv_bias'):
                v = _cfg_get(model_cfg, key)
                if v is not None:
                    config[key] = v
            v = _cfg_get(task_cfg, 'normalize')
            if v is not None:
                config['normalize'] = v
        else:
            state_dict = ckpt
        self._setup(state_dict, _load_centres(kmeans_path), target_sample_hz, seq_len_multiple_of, output_layer, config)

    @classmethod
    def from_state_dict(cls, state_dict, cluster_centers, target_sample_hz=16000, seq_len_multiple_of=None, output_layer=9, **config):
        """builds the module from a fairseq-named state dict and a (clusters, dim) array, no files.  `config`: conv_feature_layers (fairseq's string
        or a list of (dim, kernel, stride); default the base stack), encoder_attention_heads (default dim / 64), conv_pos_groups (16), and the
        options that raise when set: layer_norm_first, extractor_mode='layer_norm', normalize, conv_bias."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._setup(state_dict, cluster_centers, target_sample_hz, seq_len_multiple_of, output_layer, dict(config))
        return self

    def _setup(self, state_dict, centres, target_sample_hz, seq_len_multiple_of, output_layer, config):
        known = {'conv_feature_layers', 'encoder_attention_heads', 'conv_pos', 'conv_pos_groups', 'layer_norm_first', 'extractor_mode', 'conv_bias', 'normalize'}
        if set(config) - known:
            raise TypeError(f'unknown configuration keys {sorted(set(config) - known)}')
        if config.get('layer_norm_first', False):
            raise NotImplementedError('layer_norm_first=True (the pre-LN large models) is not implemented: HuBERT-base only')
        if str(config.get('extractor_mode', 'default')).split('.')[-1].lower() not in ('default', 'group_norm'):
            raise NotImplementedError(f"extractor_mode={config['extractor_mode']!r} is not implemented: only the group-norm extractor ('default')")
        if config.get('normalize', False):
            raise NotImplementedError('normalize=True (wave normalisation) is not implemented')
        if config.get('conv_bias', False):
            raise NotImplementedError('conv_bias=True is not implemented')
        self.target_sample_hz = target_sample_hz
        self.seq_len_multiple_of = seq_len_multiple_of
        self.output_layer = int(output_layer)
        self.conv_layers = _conv_spec(config.get('conv_feature_layers', BASE_CONV_LAYERS))
        if self.output_layer < 1:
            raise ValueError('output_layer counts encoder layers from 1')

        names = [f'feature_extractor.conv_layers.{i}.0.weight' for i in range(len(self.conv_layers))]
        names += ['feature_extractor.conv_layers.0.2.weight', 'feature_extractor.conv_layers.0.2.bias', 'layer_norm.weight', 'layer_norm.bias',
                  'post_extract_proj.weight', 'post_extract_proj.bias', 'encoder.pos_conv.0.bias', 'encoder.pos_conv.0.weight_g',
                  'encoder.pos_conv.0.weight_v', 'encoder.layer_norm.weight', 'encoder.layer_norm.bias']
        names += [f'encoder.layers.{i}.{k}' for i in range(self.output_layer) for k in _LAYER_KEYS]
        # layers at index output_layer and above are not kept
        self._adopt(names, state_dict, f'a {self.output_layer}-layer HuBERT', lambda k: _IGNORED.match(k) or re.match(r'encoder\.layers\.(\d+)\.', k))

        sd = self._params()
        C_prev = 1
        for i, (c, k, s) in enumerate(self.conv_layers):
            w = sd[f'feature_extractor.conv_layers.{i}.0.weight']
            if tuple(w.shape) != (c, C_prev, k):
                raise ValueError(f'conv layer {i}: weight {tuple(w.shape)} does not match conv_feature_layers ({c}, {C_prev}, {k})')
            C_prev = c
        self.dim = D = sd['post_extract_proj.weight'].shape[0]
        self.heads = int(config.get('encoder_attention_heads', D // 64))
        if self.heads * 64 != D:
            raise NotImplementedError(f'head width {D / self.heads:g} is not implemented: heads of width 64 only (dim {D}, {self.heads} heads)')
        self.conv_pos_groups = int(config.get('conv_pos_groups', 16))
        wv = sd['encoder.pos_conv.0.weight_v']
        self.conv_pos = wv.shape[2]
        if 'conv_pos' in config and int(config['conv_pos']) != self.conv_pos:
            raise ValueError(f"conv_pos={config['conv_pos']} but the positional conv weight has {self.conv_pos} taps")
        if wv.shape[0] != D or wv.shape[1] * self.conv_pos_groups != D:
            raise ValueError(f'positional conv weight {tuple(wv.shape)} does not match dim {D} in {self.conv_pos_groups} groups')

        centres = torch.as_tensor(centres).detach().to(F32).contiguous()
        if centres.dim() != 2 or centres.shape[1] != D:
            raise ValueError(f'cluster centres must be (clusters, {D}), got {tuple(centres.shape)}')
        self.register_buffer('cluster_centers', centres.clone())
        self._fold()
        self.eval()

    def _fold(self):
        """derived tensors, computed once at load: the positional conv's weight norm folded (w = g v / |v|, the norm over all but the tap axis,
        torch.nn.utils.weight_norm(dim=2)), the q | k | v projections stacked for one launch"""
        p = self._params()
        g, v = p['encoder.pos_conv.0.weight_g'], p['encoder.pos_conv.0.weight_v']
        self.register_buffer('_pos_w', (v * (g / v.norm(dim=(0, 1), keepdim=True))).contiguous(), persistent=False)
        for i in range(self.output_layer):
            pre = f'encoder.layers.{i}.self_attn.'
            self.register_buffer(f'_qkv_w{i}', torch.cat([p[pre + f'{n}_proj.weight'] for n in 'qkv']).unsqueeze(-1).contiguous(), persistent=False)
            self.register_buffer(f'_qkv_b{i}', torch.cat([p[pre + f'{n}_proj.bias'] for n in 'qkv']).contiguous(), persistent=False)

    @property
    def groups(self):
        return 1

    @property
    def codebook_size(self):
        return self.cluster_centers.shape[0]

    @property
    def downsample_factor(self):
        return 320

    def _check(self, wav_input, padding_mask):
        if padding_mask is not None:
            raise NotImplementedError('padding_mask is not implemented: rows of one batch share one length')
        if not wav_input.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.HubertWithKmeans runs on the MI355X only (no CPU fallback)')
        if wav_input.dim() != 2:
            raise ValueError(f'wav_input must be (batch, samples), got {tuple(wav_input.shape)}')

    @torch.no_grad()
    def features(self, wav_input, padding_mask=None):
        """wave (b, t) at target_sample_hz -> the output of encoder layer `output_layer`, fp32 (b, n, dim): what fairseq returns as
        model(wav, features_only=True, mask=False, output_layer=L)['x']"""
        self._check(wav_input, padding_mask)
        p, lin = self._params(), self._linear
        x = wav_input.to(F32)
        c0, k0, s0 = self.conv_layers[0]
        w0 = p['feature_extractor.conv_layers.0.0.weight'].view(c0, k0)
        stats = ops.hubert_conv0_stats(x, w0, s0, eps=1e-5)
        x = ops.hubert_conv0_apply(x, w0, stats, p['feature_extractor.conv_layers.0.2.weight'], p['feature_extractor.conv_layers.0.2.bias'], s0)
        for i, (_, _, s) in enumerate(self.conv_layers[1:], 1):
            x = ops.conv1d_valid(x, p[f'feature_extractor.conv_layers.{i}.0.weight'], stride=s, gelu=True)
        x = ops.layernorm_bct_split(x, p['layer_norm.weight'], p['layer_norm.bias'], eps=1e-5)
        x = ops.conv1d_valid(x, lin('post_extract_proj.weight'), p['post_extract_proj.bias'])
        # pos_conv pads conv_pos // 2 on both sides; SamePad drops the last output of an even kernel; x = x + gelu(.)
        x = ops.conv1d_valid(x, self._pos_w, p['encoder.pos_conv.0.bias'], pad=self.conv_pos // 2, groups=self.conv_pos_groups, gelu=True, residual=x,
                             drop_last=1 if self.conv_pos % 2 == 0 else 0)
        x = ops.layernorm_bct_split(x, p['encoder.layer_norm.weight'], p['encoder.layer_norm.bias'], eps=1e-5)
        for i in range(self.output_layer):
            pre = f'encoder.layers.{i}.'
            qkv = ops.conv1d_valid(x, getattr(self, f'_qkv_w{i}'), getattr(self, f'_qkv_b{i}'))
            a = ops.mha_attn(qkv, self.heads)
            x = ops.conv1d_valid(a, lin(pre + 'self_attn.out_proj.weight'), p[pre + 'self_attn.out_proj.bias'], residual=x)
            x = ops.layernorm_bct_split(x, p[pre + 'self_attn_layer_norm.weight'], p[pre + 'self_attn_layer_norm.bias'], eps=1e-5)
            h = ops.conv1d_valid(x, lin(pre + 'fc1.weight'), p[pre + 'fc1.bias'], gelu=True)
            x = ops.conv1d_valid(h, lin(pre + 'fc2.weight'), p[pre + 'fc2.bias'], residual=x)
            x = ops.layernorm_bct_split(x, p[pre + 'final_layer_norm.weight'], p[pre + 'final_layer_norm.bias'], eps=1e-5)
        return ops.bct_to_btc(x)

    @torch.no_grad()
    def assign(self, embed):
        """fp32 (b, n, dim) -> long (b, n): (-cdist(embed, centres)).argmax(-1), the first index on ties (hubert_kmeans.py:114-116)"""
        b, n, d = embed.shape
        E = self.cluster_centers.unsqueeze(0)
        ids = ops.rvq_encode(embed.reshape(b * n, d), E, *self._cached('centre_image', lambda: ops.rvq_pack(E)))
        return ids.view(b, n)

    @torch.no_grad()
    def forward(self, wav_input, flatten=True, input_sample_hz=None, padding_mask=None):
        self._check(wav_input, padding_mask)
        if input_sample_hz is not None:
            wav_input = resample(wav_input, input_sample_hz, self.target_sample_hz)
        if self.seq_len_multiple_of is not None:
            wav_input = curtail_to_multiple(wav_input, self.seq_len_multiple_of)
        clusters = self.assign(self.features(wav_input))
        if flatten:
            return clusters
        return clusters.reshape(clusters.shape[0], -1)          # 'b ... -> b (...)': the same (b, n) for a (b, t) wave, as in the reference


def _load_centres(path):
    path = str(path)
    if path.endswith('.pt'):
        c = load_weights(path)
        return c['cluster_centers'] if isinstance(c, dict) else c
    if path.endswith('.npy'):
        import numpy as np
        return torch.from_numpy(np.load(path))
    import joblib
    km = joblib.load(path)
    if not hasattr(km, 'cluster_centers_'):
        raise ValueError(f'{path} holds a {type(km).__name__} without cluster_centers_')
    return torch.from_numpy(km.cluster_centers_)
