"""The T5 encoder (transformers T5Stack, encoder only) and the reference's t5_encode_text masking, restated in plain torch as test infrastructure.

This is the oracle that audiolm-pytorch_amd/t5.py + csrc/t5.hip are checked against; it is written from the published architecture (shared embedding,
pre-norm blocks: T5LayerNorm -> self-attention with a bucketed relative-position bias, no 1 / sqrt(d) scale -> residual; T5LayerNorm -> relu or
gated gelu_new feed-forward -> residual; final T5LayerNorm), runs from a transformers-named state dict and nothing here imports the product.  `dtype`
selects the arithmetic: fp32 is what transformers computes, fp64 the high-precision yardstick.  tests/test_t5_host.py pins it to a forward recorded
from transformers.T5EncoderModel in fp64 (tests/golden/t5_tiny.pt).
"""
import math

import torch
import torch.nn.functional as F

BIAS_KEY = 'encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight'
# gain of the o / wo weights of random_state_dict: the branches add about a third of the residual stream's variance per block, so a token keeps
# its identity through twelve blocks and the stream stays O(1..5), the scale of the published checkpoints' hidden states
BRANCH_GAIN = 0.55


def random_state_dict(seed, d_model=768, layers=12, heads=12, d_ff=2048, vocab=512, gated=True, num_buckets=32, dtype=torch.float32):
    """seeded transformers-named weights with sensible scales (scores O(1) without the 1 / sqrt(d) factor T5 folds into its weights)"""
    g = torch.Generator().manual_seed(seed)
    inner = heads * 64

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)
    sd = {'shared.weight': rn(vocab, d_model), BIAS_KEY: rn(num_buckets, heads)}
    for i in range(layers):
        a, f = f'encoder.block.{i}.layer.0.', f'encoder.block.{i}.layer.1.'
        for n in 'qk':
            sd[a + f'SelfAttention.{n}.weight'] = rn(inner, d_model, scale=0.45 * d_model ** -0.5)       # q . k over 64 terms: std ~ 1.6
        sd[a + 'SelfAttention.v.weight'] = rn(inner, d_model, scale=d_model ** -0.5)
        sd[a + 'SelfAttention.o.weight'] = rn(d_model, inner, scale=BRANCH_GAIN * inner ** -0.5)
        sd[a + 'layer_norm.weight'] = 1 + rn(d_model, scale=0.1)
        for n in (('wi_0', 'wi_1') if gated else ('wi',)):
            sd[f + f'DenseReluDense.{n}.weight'] = rn(d_ff, d_model, scale=d_model ** -0.5)
        sd[f + 'DenseReluDense.wo.weight'] = rn(d_model, d_ff, scale=BRANCH_GAIN * d_ff ** -0.5)
        sd[f + 'layer_norm.weight'] = 1 + rn(d_model, scale=0.1)
    sd['encoder.final_layer_norm.weight'] = 1 + rn(d_model, scale=0.1)
    return sd


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5's bidirectional bucket of key - query (int64 tensor): half the buckets per sign; the first half of those exact, the rest logarithmic up to
    max_distance.  The logarithm is taken in fp32, as transformers takes it: the recorded indices of tests/golden/t5_tiny.pt pin every rounding."""
    half = num_buckets // 2
    out = (relative_position > 0).to(torch.long) * half
    n = relative_position.abs()
    exact = half // 2
    large = exact + (torch.log(n.float() / exact) / math.log(max_distance / exact) * (half - exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, half - 1))
    return out + torch.where(n < exact, n, large)


def position_bias(table, T, num_buckets=32, max_distance=128):
    """table [num_buckets, H] -> [H, T, T]: bias[h, i, j] = table[bucket(j - i), h]"""
    pos = torch.arange(T)
    return table[relative_position_bucket(pos[None, :] - pos[:, None], num_buckets, max_distance)].permute(2, 0, 1)


def rms_norm(x, w, eps=1e-6):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def gelu_new(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u.pow(3))))


def attention(q, k, v, bias, mask, heads):
    """q, k, v [B, n, H 64] (no scale), bias [H, n, n], mask [B, n] bool (True = a key that counts) -> [B, n, H 64].  A masked key gets the
    dtype's most negative number added, as transformers does: probability exactly 0 as long as one key of the row counts."""
    B, n, inner = q.shape
    split = lambda t: t.view(B, n, heads, inner // heads).transpose(1, 2)                      # noqa: E731
    s = split(q) @ split(k).transpose(-1, -2) + bias[None]
    s = s + (~mask)[:, None, None, :].to(s.dtype) * torch.finfo(s.dtype).min
    return (torch.softmax(s, dim=-1) @ split(v)).transpose(1, 2).reshape(B, n, inner)


def hidden_states(sd, ids, mask=None, heads=12, gated=True, num_buckets=32, max_distance=128, eps=1e-6, dtype=torch.float32, bias=None):
    """ids [B, n] long, mask [B, n] (0 / 1) -> last_hidden_state [B, n, d_model] of T5EncoderModel(input_ids=ids, attention_mask=mask) in eval mode.
    bias: a position_bias(...) tensor already on ids' device (a timing loop builds it once, as transformers builds it on the device)"""
    W = lambda name: sd[name].to(dtype)                                                        # noqa: E731
    B, n = ids.shape
    mask = torch.ones(B, n, dtype=torch.bool) if mask is None else mask.to(ids.device) != 0
    layers = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('encoder.block.'))
    if bias is None:
        bias = position_bias(W(BIAS_KEY).cpu(), n, num_buckets, max_distance).to(ids.device)
    x = W('shared.weight')[ids]
    for i in range(layers):
        a, f = f'encoder.block.{i}.layer.0.', f'encoder.block.{i}.layer.1.DenseReluDense.'
        h = rms_norm(x, W(a + 'layer_norm.weight'), eps)
        lin = lambda n_: F.linear(h, W(a + f'SelfAttention.{n_}.weight'))                      # noqa: E731
        x = x + F.linear(attention(lin('q'), lin('k'), lin('v'), bias, mask, heads), W(a + 'SelfAttention.o.weight'))
        h = rms_norm(x, W(f'encoder.block.{i}.layer.1.layer_norm.weight'), eps)
        if gated:
            u = gelu_new(F.linear(h, W(f + 'wi_0.weight'))) * F.linear(h, W(f + 'wi_1.weight'))
        else:
            u = torch.relu(F.linear(h, W(f + 'wi.weight')))
        x = x + F.linear(u, W(f + 'wo.weight'))
    return rms_norm(x, W('encoder.final_layer_norm.weight'), eps)


def encode(sd, ids, mask=None, **kw):
    """reference t5.py:94-110: the encoder's last hidden state with the padded positions filled with zeros"""
    out = hidden_states(sd, ids, mask, **kw)
    if mask is None:
        return out
    return out.masked_fill(~(mask.to(out.device) != 0)[..., None], 0.)


class StubTokenizer:
    """stands in for transformers.T5Tokenizer in tests: one id per whitespace-separated word (a stable hash into [2, vocab)), id 1 appended as
    </s>, padded with id 0 to the longest row; called exactly as t5_encode_text calls the real one"""

    def __init__(self, vocab):
        self.vocab, self.calls = vocab, 0

    def __call__(self, texts, return_tensors='pt', padding='longest', max_length=None, truncation=True):
        assert return_tensors == 'pt' and padding == 'longest' and truncation is True and isinstance(texts, list)
        self.calls += 1
        rows = []
        for t in texts:
            ids = [2 + sum(ord(c) * (i + 1) for i, c in enumerate(w)) % (self.vocab - 2) for w in t.split()][:max_length - 1] + [1]
            rows.append(ids)
        n = max(len(r) for r in rows)
        out = type('Encoding', (), {})()
        out.input_ids = torch.tensor([r + [0] * (n - len(r)) for r in rows], dtype=torch.long)
        out.attention_mask = torch.tensor([[1] * len(r) + [0] * (n - len(r)) for r in rows], dtype=torch.long)
        return out
