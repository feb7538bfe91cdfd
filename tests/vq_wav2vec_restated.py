"""fairseq's vq-wav2vec (Wav2VecModel with vq_type='kmeans') as the reference's FairseqVQWav2Vec calls it, restated in plain torch as test infrastructure.

fairseq is not available to this project.  This is the oracle that audiolm-pytorch_amd/vq_wav2vec.py + csrc/vq_wav2vec.hip are checked against; it is
written from the published model definition (ConvFeatureExtractionModel: conv + GroupNorm(1, C) + ReLU per layer, optional skip connections and log
compression; KmeansVectorQuantizer.forward_idx: grouped 1x1 projection + GroupNorm(groups, C), nearest code per group), runs from a fairseq-named
state dict and nothing here imports the product.  `dtype` selects the arithmetic: fp32 is what fairseq computes, fp64 the high-precision yardstick.
Parity with the installed fairseq package is not pinned (it is not installed here).
"""
import math

import torch
import torch.nn.functional as F

RELEASED_CONV = [(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), (512, 1, 1), (512, 1, 1)]


def frame_count(T, conv=RELEASED_CONV):
    for _, k, s in conv:
        T = (T - k) // s + 1 if T >= k else 0
    return T


def random_state_dict(seed, conv=RELEASED_CONV, groups=2, num_vars=320, combine_groups=False, affine=True, dtype=torch.float32):
    """seeded fairseq-named weights: He-scaled convs (activations stay O(1) through the ReLU stack), a projection of gain 1 per group, norm weights
    near 1 and biases near 0.  The embedding is fairseq's initial 0.01 randn; the tests that assign replace it (all codes at the origin decide
    nothing)."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)
    sd = {}
    cin = 1
    for i, (c, k, s) in enumerate(conv):
        sd[f'feature_extractor.conv_layers.{i}.0.weight'] = rn(c, cin, k, scale=math.sqrt(2.0 / (cin * k)))
        if affine:
            sd[f'feature_extractor.conv_layers.{i}.2.weight'] = 1 + rn(c, scale=0.1)
            sd[f'feature_extractor.conv_layers.{i}.2.bias'] = rn(c, scale=0.1)
        cin = c
    C = cin
    sd['vector_quantizer.projection.0.weight'] = rn(C, C // groups, 1, scale=math.sqrt(groups / C))
    sd['vector_quantizer.projection.1.weight'] = 1 + rn(C, scale=0.1)
    sd['vector_quantizer.projection.1.bias'] = rn(C, scale=0.1)
    sd['vector_quantizer.embedding'] = rn(num_vars, 1 if combine_groups else groups, C // groups, scale=0.01)
    return sd


def groups_of(sd):
    w = sd['vector_quantizer.projection.0.weight']
    return w.shape[0] // w.shape[1]


def feature_extractor(sd, wave, dtype=torch.float32, conv=RELEASED_CONV, log_compression=True, skip_connections=False, residual_scale=0.5, eps=1e-5):
    """ConvFeatureExtractionModel.forward: wave [B, T] -> [B, C, T']"""
    x = wave.to(dtype)[:, None]
    scale = math.sqrt(residual_scale)
    for i, (c, k, s) in enumerate(conv):
        residual = x
        x = F.conv1d(x, sd[f'feature_extractor.conv_layers.{i}.0.weight'].to(dtype), stride=s)
        gamma, beta = sd.get(f'feature_extractor.conv_layers.{i}.2.weight'), sd.get(f'feature_extractor.conv_layers.{i}.2.bias')
        x = F.relu(F.group_norm(x, 1, None if gamma is None else gamma.to(dtype), None if beta is None else beta.to(dtype), eps))
        if skip_connections and x.shape[1] == residual.shape[1]:
            tsz, r_tsz = x.shape[2], residual.shape[2]
            residual = residual[..., ::r_tsz // tsz][..., :tsz]
            x = (x + residual) * scale
    if log_compression:
        x = (x.abs() + 1).log()
    return x


def quantizer_head(sd, x, dtype=torch.float32, eps=1e-5):
    """KmeansVectorQuantizer.forward_idx up to the distance: x [B, C, T] -> ze_ [B, T, groups, var_dim]"""
    G = groups_of(sd)
    ze = F.conv1d(x, sd['vector_quantizer.projection.0.weight'].to(dtype), groups=G)
    ze = F.group_norm(ze, G, sd['vector_quantizer.projection.1.weight'].to(dtype), sd['vector_quantizer.projection.1.bias'].to(dtype), eps)
    B, C, T = ze.shape
    return ze.view(B, G, C // G, T).permute(0, 3, 1, 2)


def features(sd, wave, dtype=torch.float32, **config):
    """wave [B, T] -> ze_ [B, T', groups, var_dim]; config: conv, log_compression, skip_connections, residual_scale"""
    return quantizer_head(sd, feature_extractor(sd, wave, dtype, **config), dtype)


def codes(embedding, g):
    """group g's codebook [num_vars, var_dim] of an embedding [num_vars, groups or 1 (combine_groups), var_dim]"""
    return embedding[:, 0 if embedding.shape[1] == 1 else g]


def distances(ze, embedding):
    """exact distances by differences, [B, T', groups, num_vars]"""
    return torch.stack([(ze[:, :, g, None, :] - codes(embedding, g).to(ze.dtype)[None, None]).pow(2).sum(-1).sqrt() for g in range(ze.shape[2])], dim=2)


def assign(ze, embedding):
    """idx[b, t, g] = argmin_v |ze[b, t, g] - E[v, g]|, the first index on ties; long [B, T', groups]"""
    return distances(ze, embedding).argmin(-1)
