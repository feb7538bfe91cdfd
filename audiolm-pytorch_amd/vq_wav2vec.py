"""FairseqVQWav2Vec on the MI355X: raw wave -> grouped semantic token ids (reference vq_wav2vec.py:19-81) without fairseq.

The reference loads a fairseq vq-wav2vec checkpoint (Wav2VecModel with vq_type='kmeans') and calls two things on it, `model.feature_extractor(wav)`
and `model.vector_quantizer.forward_idx(embed)`.  Both are restated here on the project's fp32 kernels, in the codec's [B][C][T] layout:

  wave [B, T] -> conv0 (1 -> C, k 10, stride 5) + GroupNorm(1, C) + ReLU, the raw activation never stored      alm_vqw2v_conv0_stats / _apply
              -> 7 bias-less convs, each + GroupNorm(1, C) + ReLU (+ skip) ; log(|x| + 1) after the last       alm_conv1d_valid, alm_vqw2v_group_stats / _apply
              -> grouped 1x1 projection -> GroupNorm(groups, C) -> [B, T', groups, var_dim]                    alm_conv1d_valid, alm_vqw2v_group_stats / _apply_t
              -> nearest code per group, the first index on ties                                               alm_rvq_encode (one quantizer per group)

GroupNorm runs over a whole sample's (C / groups) x T block, so every id depends on whole-clip statistics; csrc/vq_wav2vec.hip takes them with centred
sums merged in a fixed order (deterministic, no E[x^2] - E[x]^2).  Parameters are registered under fairseq's key names, so the 'model' dict of a
fairseq checkpoint loads by name; the aggregator and the prediction heads are ignored.  Everything outside the documented architecture raises
NotImplementedError; a CPU tensor raises RuntimeError (there is no CPU path).
"""
from __future__ import annotations

import math
import os
import pickle
import re

import torch
from torch import nn

from . import _lib, ops
from .frozen import F32, FrozenModel
from .hubert_kmeans import _cfg_get, _conv_spec
from .resample import resample
from .soundstream import curtail_to_multiple

RELEASED_CONV_LAYERS = '[(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), (512, 1, 1), (512, 1, 1)]'
_IGNORED = re.compile(r'^(feature_aggregator\.|wav2vec_predictions\.|dropout_\w+\.)')
_CONFIG_KEYS = ('conv_feature_layers', 'log_compression', 'skip_connections_feature_extractor', 'residual_scale', 'non_affine_group_norm', 'activation',
                'vq_type', 'vq_groups', 'vq_vars', 'vq_dim', 'combine_groups')


def frame_count(num_samples, conv_layers=None):
    """frames the feature extractor gives for `num_samples` samples (the released conv stack: total stride 160, receptive field 465)"""
    n = int(num_samples)
    for _, k, s in _conv_spec(conv_layers or RELEASED_CONV_LAYERS):
        n = (n - k) // s + 1 if n >= k else 0
    return n


class FairseqVQWav2Vec(FrozenModel):
    """Positional order, defaults and members of the reference class (vq_wav2vec.py:27-60).  `checkpoint_path`: torch.load-able, a fairseq checkpoint
    ({'model': state dict, 'args': Namespace} or {'model': ..., 'cfg': {'model': ...}}) or a bare state dict."""

    def __init__(self, checkpoint_path, target_sample_hz=24000, seq_len_multiple_of=None):
        super().__init__()
        assert os.path.exists(str(checkpoint_path)), f'path {checkpoint_path} does not exist'
        try:
            ckpt = torch.load(str(checkpoint_path), map_location='cpu', weights_only=True)
        except pickle.UnpicklingError:              # fairseq checkpoints carry an argparse / omegaconf configuration object
            ckpt = torch.load(str(checkpoint_path), map_location='cpu', weights_only=False)
        config = {}
        if isinstance(ckpt, dict) and 'model' in ckpt and isinstance(ckpt['model'], dict):
            state_dict = ckpt['model']
            cfg = ckpt.get('cfg')
            model_cfg = _cfg_get(cfg, 'model') if cfg is not None else ckpt.get('args')
            for key in _CONFIG_KEYS:
                v = _cfg_get(model_cfg, key)
                if v is not None:
                    config[key] = v
        else:
            state_dict = ckpt
        self._setup(state_dict, target_sample_hz, seq_len_multiple_of, config)

    @classmethod
    def from_state_dict(cls, state_dict, target_sample_hz=24000, seq_len_multiple_of=None, **config):
        """builds the module from a fairseq-named state dict, no files.  `config`: conv_feature_layers (fairseq's string or a list of (dim, kernel,
        stride); default the released stack), log_compression (True), skip_connections_feature_extractor (False), residual_scale (0.5),
        non_affine_group_norm (False), vq_groups / vq_vars / combine_groups (default: what the tensor shapes say; checked against them when given),
        vq_dim (0 = the feature width), and the options that raise when set: vq_type='gumbel', an activation other than 'relu'."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._setup(state_dict, target_sample_hz, seq_len_multiple_of, dict(config))
        return self

    def _setup(self, state_dict, target_sample_hz, seq_len_multiple_of, config):
        if set(config) - set(_CONFIG_KEYS):
            raise TypeError(f'unknown configuration keys {sorted(set(config) - set(_CONFIG_KEYS))}')
        vq_type = str(config.get('vq_type', 'kmeans')).split('.')[-1].lower()
        if vq_type == 'gumbel':
            raise NotImplementedError("vq_type='gumbel' is not implemented: the k-means quantizer (vq-wav2vec_kmeans.pt) only")
        if vq_type != 'kmeans':
            raise ValueError(f'vq_type={config["vq_type"]!r}: not a vq-wav2vec model')
        activation = str(config.get('activation', 'relu')).split('.')[-1].lower()
        if activation != 'relu':
            raise NotImplementedError(f'activation={activation!r} is not implemented: relu only')
        self.target_sample_hz = target_sample_hz
        self.seq_len_multiple_of = seq_len_multiple_of
        self.conv_layers = _conv_spec(config.get('conv_feature_layers', RELEASED_CONV_LAYERS))
        self.log_compression = bool(config.get('log_compression', True))
        self.skip_connections = bool(config.get('skip_connections_feature_extractor', False))
        self.residual_scale = math.sqrt(float(config.get('residual_scale', 0.5)))
        self.affine = not bool(config.get('non_affine_group_norm', False))
        if self.skip_connections and self.conv_layers[0][0] == 1:
            raise NotImplementedError('a skip connection around the first conv layer (one feature channel) is not implemented')

        n_layers = len(self.conv_layers)
        names = [f'feature_extractor.conv_layers.{i}.0.weight' for i in range(n_layers)]
        if self.affine:
            names += [f'feature_extractor.conv_layers.{i}.2.{p}' for i in range(n_layers) for p in ('weight', 'bias')]
        names += ['vector_quantizer.embedding', 'vector_quantizer.projection.0.weight', 'vector_quantizer.projection.1.weight',
                  'vector_quantizer.projection.1.bias']
        self._adopt(names, state_dict, 'a vq-wav2vec model with the k-means quantizer', _IGNORED.match)

        sd = self._params()
        C_prev = 1
        for i, (c, k, s) in enumerate(self.conv_layers):
            w = sd[f'feature_extractor.conv_layers.{i}.0.weight']
            if tuple(w.shape) != (c, C_prev, k):
                raise ValueError(f'conv layer {i}: weight {tuple(w.shape)} does not match conv_feature_layers ({c}, {C_prev}, {k})')
            if self.affine and tuple(sd[f'feature_extractor.conv_layers.{i}.2.weight'].shape) != (c,):
                raise ValueError(f'conv layer {i}: the norm weight is not ({c},)')
            C_prev = c
        self.dim = C = C_prev
        vq_dim = int(config.get('vq_dim', 0))
        if vq_dim not in (0, C):
            raise NotImplementedError(f'vq_dim={vq_dim} is not implemented: 0 or the feature width {C}')
        E, pw = sd['vector_quantizer.embedding'], sd['vector_quantizer.projection.0.weight']
        if pw.dim() != 3 or pw.shape[0] != C or pw.shape[2] != 1 or pw.shape[1] == 0 or C % pw.shape[1]:
            raise ValueError(f'the quantizer projection weight {tuple(pw.shape)} is not ({C}, {C} / groups, 1)')
        self._groups = C // pw.shape[1]
        var_dim = C // self._groups
        if E.dim() != 3 or E.shape[1] not in (1, self._groups) or E.shape[2] != var_dim:
            raise ValueError(f'the embedding {tuple(E.shape)} is not (num_vars, {self._groups} or 1, {var_dim})')
        self.combine_groups = self._groups > 1 and E.shape[1] == 1
        for key, have in (('vq_groups', self._groups), ('vq_vars', E.shape[0])):
            if key in config and int(config[key]) != have:
                raise ValueError(f'{key}={config[key]} but the tensors say {have}')
        if 'combine_groups' in config and self._groups > 1 and bool(config['combine_groups']) != self.combine_groups:
            raise ValueError(f"combine_groups={config['combine_groups']} but the embedding is {tuple(E.shape)}")
        if tuple(sd['vector_quantizer.projection.1.weight'].shape) != (C,):
            raise ValueError(f'the quantizer norm weight is not ({C},)')
        self.eval()

    @property
    def groups(self):
        return self._groups

    @property
    def downsample_factor(self):
        return 80            # the reference's constant (vq_wav2vec.py:54-56, 'todo: double check architecture'), kept as it is

    @property
    def codebook_size(self):
        return self._params()['vector_quantizer.embedding'].shape[0]

    def _check(self, wav_input):
        if not wav_input.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.FairseqVQWav2Vec runs on the MI355X only (no CPU fallback)')
        if wav_input.dim() != 2:
            raise ValueError(f'wav_input must be (batch, samples), got {tuple(wav_input.shape)}')

    def _norm(self, i, C, device):
        """(gamma, beta) of conv layer i; ones / zeros for non-affine norms"""
        if self.affine:
            p = self._params()
            return p[f'feature_extractor.conv_layers.{i}.2.weight'], p[f'feature_extractor.conv_layers.{i}.2.bias']
        return self._cached(('identity', C), lambda: (torch.ones(C, dtype=F32, device=device), torch.zeros(C, dtype=F32, device=device)))

    @torch.no_grad()
    def features(self, wav_input):
        """wave (b, t) at target_sample_hz -> ze, fp32 (b, n, groups, var_dim): the projected, group-normalised features the codes are searched
        with (KmeansVectorQuantizer.forward_idx up to the distance)"""
        self._check(wav_input)
        if frame_count(wav_input.shape[1], self.conv_layers) < 1:
            raise _lib.AlmError(f'the wave has {wav_input.shape[1]} samples: too short for one frame of the feature extractor')
        p = self._params()
        x = wav_input.to(F32)
        last = len(self.conv_layers) - 1
        c0, k0, s0 = self.conv_layers[0]
        w0 = p['feature_extractor.conv_layers.0.0.weight'].view(c0, k0)
        g, b = self._norm(0, c0, x.device)
        x = ops.vqw2v_conv0_apply(x, w0, ops.vqw2v_conv0_stats(x, w0, s0), g, b, s0, log_compression=self.log_compression and last == 0)
        for i, (c, _, s) in enumerate(self.conv_layers[1:], 1):
            y = ops.conv1d_valid(x, p[f'feature_extractor.conv_layers.{i}.0.weight'], stride=s)
            g, b = self._norm(i, c, x.device)
            skip = self.skip_connections and c == x.shape[1]
            x = ops.vqw2v_group_apply(y, ops.vqw2v_group_stats(y, 1), g, b, relu=True, residual=x if skip else None,
                                      residual_scale=self.residual_scale, log_compression=self.log_compression and i == last)
        z = ops.conv1d_valid(x, p['vector_quantizer.projection.0.weight'], groups=self._groups)
        ze = ops.vqw2v_group_apply_t(z, ops.vqw2v_group_stats(z, self._groups), p['vector_quantizer.projection.1.weight'],
                                     p['vector_quantizer.projection.1.bias'])
        return ze.view(ze.shape[0], ze.shape[1], self._groups, -1)

    def _codebook(self, g):
        """group g's codes as a one-quantizer codebook [1, num_vars, var_dim] and its packed image (one shared codebook with combine_groups)"""
        g = 0 if self.combine_groups else g

        def make():
            E = self._params()['vector_quantizer.embedding'][:, g].contiguous().unsqueeze(0)
            return (E, *ops.rvq_pack(E))
        return self._cached(('codebook', g), make)

    @torch.no_grad()
    def assign(self, ze):
        """fp32 (b, n, groups, var_dim) -> long (b, n, groups): argmin_v |ze[b, t, g] - E[v, g]|, the first index on ties"""
        b, n, G, V = ze.shape
        assert G == self._groups
        rows = ze.to(F32).contiguous().view(b * n, G * V)
        idx = torch.empty((b * n, G), dtype=torch.int64, device=ze.device)
        for g in range(G):
            ops.rvq_encode(rows[:, g * V:(g + 1) * V], *self._codebook(g), idx_out=idx[:, g:g + 1])
        return idx.view(b, n, G)

    @torch.no_grad()
    def forward(self, wav_input, flatten=True, input_sample_hz=None):
        self._check(wav_input)
        if input_sample_hz is not None:
            wav_input = resample(wav_input, input_sample_hz, self.target_sample_hz)
        if self.seq_len_multiple_of is not None:
            wav_input = curtail_to_multiple(wav_input, self.seq_len_multiple_of)
        codebook_indices = self.assign(self.features(wav_input))
        if not flatten:
            return codebook_indices
        return codebook_indices.reshape(codebook_indices.shape[0], -1)          # 'b ... -> b (...)': time-major, the groups interleaved
