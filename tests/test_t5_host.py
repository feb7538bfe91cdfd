"""CPU: the host side of audiolm_pytorch_amd.T5Encoder / t5_encode_text and the restated T5 encoder (tests/t5_restated.py) it is checked against on
the GPU.

The restatement is pinned in fp64 to forwards recorded from transformers.T5EncoderModel (tests/golden/t5_tiny.pt, written by
tests/golden/make_t5_golden.py): a gated-gelu and a relu config, ragged masks.  The bucket table, loading, the key checks, the refusals, the
registry and the reference import path need no GPU.  No kernel runs here."""
import json
import os
import sys

import pytest
import torch

import t5_restated as TR
import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import t5 as T5
from common import GOLDEN_DIR


def tiny():
    return torch.load(os.path.join(GOLDEN_DIR, 't5_tiny.pt'), weights_only=True)


def kw_of(cfg):
    return dict(num_heads=cfg['num_heads'], d_kv=cfg['d_kv'], feed_forward_proj=cfg['feed_forward_proj'],
                relative_attention_num_buckets=cfg['relative_attention_num_buckets'],
                relative_attention_max_distance=cfg['relative_attention_max_distance'], layer_norm_epsilon=cfg['layer_norm_epsilon'])


def restated_kw(cfg, dtype):
    return dict(heads=cfg['num_heads'], gated=cfg['feed_forward_proj'] == 'gated-gelu', num_buckets=cfg['relative_attention_num_buckets'],
                max_distance=cfg['relative_attention_max_distance'], eps=cfg['layer_norm_epsilon'], dtype=dtype)


@pytest.mark.parametrize('name', ['gated', 'relu'])
def test_restatement_reproduces_the_recorded_transformers_forward(name):
    """fp64 against fp64: the same arithmetic up to summation order -> per-position L2 error <= 1e-9 of the position's norm; padded positions 0"""
    t = tiny()[name]
    got = TR.encode(t['state_dict'], t['ids'], t['mask'], **restated_kw(t['config'], torch.float64))
    want = t['output64']
    assert got.shape == want.shape == (4, 40, t['config']['d_model']) and want.dtype == torch.float64
    valid = t['mask'].bool()
    rel = (got - want).norm(dim=-1)[valid] / want.norm(dim=-1)[valid]
    print(f'{name}: restatement vs recorded transformers forward, max relative L2 per position {float(rel.max()):.3e}')
    assert float(rel.max()) <= 1e-9
    assert bool((got[~valid] == 0).all()) and bool((want[~valid] == 0).all())
    assert {int(m.sum()) for m in t['mask']} == {40, 1, 17, 26}                     # the fixture's rows: full, one token, prefix, non-prefix


@pytest.mark.parametrize('name', ['gated', 'relu'])
def test_restatement_agrees_with_the_unpatched_transformers_model(name):
    """the recording above comes from a model whose norm modules were given an fp64 variance; this one is transformers exactly as shipped, whose
    T5LayerNorm rounds the hidden state to fp32 and takes the mean of d_model squares in fp32: each of the 2 L + 1 = 5 norms on the path carries at
    most (d_model + 2) u in its rstd (u = 2^-24), so the two forwards differ by at most 5 (d_model + 2) u of a position's norm to first order"""
    t = tiny()[name]
    got = TR.encode(t['state_dict'], t['ids'], t['mask'], **restated_kw(t['config'], torch.float64))
    want, valid = t['output_unpatched'], t['mask'].bool()
    rel = float(((got - want).norm(dim=-1)[valid] / want.norm(dim=-1)[valid]).max())
    bound = 5 * (t['config']['d_model'] + 2) * 2.0 ** -24
    print(f'{name}: restatement vs unpatched transformers, max relative L2 per position {rel:.3e} (bound {bound:.3e})')
    assert rel <= bound


@pytest.mark.parametrize('nb, md', [(32, 128), (16, 40)])
def test_bucket_indices_equal_the_recorded_ones(nb, md):
    t = tiny()
    want = t['buckets'][f'{nb},{md}'].to(torch.long)
    assert t['delta'].tolist() == list(range(-600, 601))
    assert torch.equal(T5.relative_position_bucket(t['delta'], nb, md), want)
    assert torch.equal(TR.relative_position_bucket(t['delta'], nb, md), want)
    assert int(want.min()) == 0 and int(want.max()) == nb - 1


def test_bias_table_is_the_dense_bias_by_delta():
    t = tiny()['gated']
    enc = A.T5Encoder.from_state_dict(t['state_dict'], **kw_of(t['config']))
    for T in (1, 7, 40, 300):
        tbl = enc.bias_table(T, 'cpu')
        assert tbl.shape == (2, 2 * T - 1) and tbl.is_contiguous()
        dense = TR.position_bias(t['state_dict'][TR.BIAS_KEY], T)                  # [H, i, j]
        i, j = torch.meshgrid(torch.arange(T), torch.arange(T), indexing='ij')
        assert torch.equal(tbl[:, (j - i + T - 1)], dense)
        assert enc.bias_table(T, 'cpu') is tbl                                      # built once per (T, device)


def test_parameter_names_state_dict_and_refold():
    t = tiny()['gated']
    sd = t['state_dict']
    enc = A.T5Encoder.from_state_dict(sd, **kw_of(t['config']))
    assert set(enc.state_dict()) == set(sd)                                         # transformers' names, derived tensors not persistent
    assert (enc.d_model, enc.num_layers, enc.num_heads, enc.d_ff, enc.vocab_size) == (64, 2, 2, 64, 50)
    assert not any(p.requires_grad for p in enc.parameters()) and not enc.training
    pre = 'encoder.block.1.layer.'
    assert torch.equal(enc._qkv_w1[:, :, 0], torch.cat([sd[pre + f'0.SelfAttention.{n}.weight'] for n in 'qkv']))
    assert torch.equal(enc._wi_w1[:, :, 0], torch.cat([sd[pre + f'1.DenseReluDense.{n}.weight'] for n in ('wi_0', 'wi_1')]))
    other = TR.random_state_dict(9, d_model=64, layers=2, heads=2, d_ff=64, vocab=50)
    tbl = enc.bias_table(5, 'cpu')
    enc.load_state_dict(other)                                                      # derived tensors follow the new weights
    assert torch.equal(enc._qkv_w0[:, :, 0], torch.cat([other[f'encoder.block.0.layer.0.SelfAttention.{n}.weight'] for n in 'qkv']))
    assert enc.bias_table(5, 'cpu') is not tbl
    assert torch.equal(enc.bias_table(5, 'cpu')[:, 4], other[TR.BIAS_KEY][0])


def test_alias_ignored_keys_and_key_errors():
    t = tiny()['gated']
    sd, kw = t['state_dict'], kw_of(t['config'])
    full = dict(sd)
    full['encoder.embed_tokens.weight'] = sd['shared.weight']
    full['decoder.block.0.layer.0.SelfAttention.q.weight'] = torch.zeros(2, 2)
    full['lm_head.weight'] = torch.zeros(2, 2)
    enc = A.T5Encoder.from_state_dict(full, **kw)
    assert set(enc.state_dict()) == set(sd)
    alias_only = {k: v for k, v in full.items() if k != 'shared.weight'}
    assert torch.equal(A.T5Encoder.from_state_dict(alias_only, **kw).state_dict()['shared.weight'], sd['shared.weight'])
    lacking = {k: v for k, v in sd.items() if k != 'encoder.block.1.layer.1.DenseReluDense.wi_1.weight'}
    with pytest.raises(KeyError, match='wi_1'):
        A.T5Encoder.from_state_dict(lacking, **kw)
    with pytest.raises(KeyError, match='surprise'):
        A.T5Encoder.from_state_dict({**sd, 'encoder.surprise.weight': torch.zeros(1)}, **kw)
    with pytest.raises(KeyError, match=r'DenseReluDense\.wi\.weight'):             # a gated state dict is not a relu model
        A.T5Encoder.from_state_dict(sd, **{**kw, 'feed_forward_proj': 'relu'})


def test_refusals():
    t = tiny()['gated']
    sd, kw = t['state_dict'], kw_of(t['config'])
    with pytest.raises(NotImplementedError, match='d_kv'):
        A.T5Encoder.from_state_dict(sd, **{**kw, 'd_kv': 128})
    with pytest.raises(NotImplementedError, match='feed_forward_proj'):
        A.T5Encoder.from_state_dict(sd, **{**kw, 'feed_forward_proj': 'gated-silu'})
    with pytest.raises(NotImplementedError, match='is_decoder'):
        A.T5Encoder.from_state_dict(sd, is_decoder=True, **kw)
    with pytest.raises(TypeError):
        A.T5Encoder.from_state_dict(sd, tie_word_embeddings=True, **kw)
    enc = A.T5Encoder.from_state_dict(sd, **kw)
    with pytest.raises(RuntimeError, match='MI355X'):
        enc(t['ids'], t['mask'])                                                    # CPU tensor: no CPU path


@pytest.mark.parametrize('fmt', ['safetensors', 'bin'])
def test_from_pretrained_round_trips_a_local_directory(tmp_path, fmt):
    t = tiny()['relu']
    cfg, sd = t['config'], t['state_dict']
    with open(tmp_path / 'config.json', 'w') as fh:
        json.dump({**cfg, 'model_type': 't5', 'architectures': ['T5EncoderModel']}, fh)
    full = {**sd, 'encoder.embed_tokens.weight': sd['shared.weight'].clone()}
    if fmt == 'safetensors':
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in full.items()}, str(tmp_path / 'model.safetensors'))
    else:
        torch.save(full, tmp_path / 'pytorch_model.bin')
    enc = A.T5Encoder.from_pretrained(str(tmp_path))
    assert not enc.gated and (enc.num_buckets, enc.max_distance, enc.num_heads) == (16, 40, 1)
    got = enc.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_from_pretrained_never_resolves_a_name(tmp_path):
    before = 'transformers' in sys.modules
    with pytest.raises(FileNotFoundError, match='local'):
        A.T5Encoder.from_pretrained('google/t5-v1_1-base')
    with pytest.raises(FileNotFoundError):
        A.load_t5('google/t5-v1_1-base', str(tmp_path / 'absent'))
    assert ('transformers' in sys.modules) == before                                # the refusal does not go through transformers
    with pytest.raises(FileNotFoundError, match='neither'):
        (tmp_path / 'config.json').write_text(json.dumps({'num_heads': 1}))
        A.T5Encoder.from_pretrained(str(tmp_path))


def test_registry_rules():
    t = tiny()['gated']
    enc = A.T5Encoder.from_state_dict(t['state_dict'], **kw_of(t['config']))
    name = 'local/t5-host-test'
    assert T5.MAX_LENGTH == 256 and T5.DEFAULT_T5_NAME == 'google/t5-v1_1-base'
    with pytest.raises(NotImplementedError, match='register'):
        A.t5_encode_text(['a dog barking'], name=name)
    with pytest.raises(NotImplementedError, match='text_embeds'):
        A.t5_encode_text('a dog barking')                                           # the default name is not registered either
    assert T5.get_encoded_dim(name) == 768 and T5.get_encoded_dim('t5-small') == 512 and T5.get_encoded_dim('google/t5-v1_1-large') == 1024
    with pytest.raises(TypeError):
        A.register_t5(name, object(), TR.StubTokenizer(50))
    try:
        assert A.register_t5(name, enc, TR.StubTokenizer(50)) is enc
        assert T5.get_encoded_dim(name) == 64
        m = A.SemanticTransformer(dim=32, depth=1, num_semantic_tokens=10, has_condition=True, t5_name=name)
        assert tuple(m.proj_text_embed.weight.shape) == (32, 64)                    # built from the registered encoder's d_model
        assert m.embed_text.keywords == {'name': name} and m.embed_text.func is A.t5_encode_text
        with pytest.raises(RuntimeError, match='MI355X'):                           # registered: the call reaches the encoder, which has no CPU path
            m.embed_text(['a dog barking'])
    finally:
        T5.unregister_t5(name)
    with pytest.raises(NotImplementedError):
        A.t5_encode_text(['a dog barking'], name=name)
    unreg = A.CoarseTransformer(dim=32, depth=1, num_semantic_tokens=10, codebook_size=8, num_coarse_quantizers=2, has_condition=True)
    assert tuple(unreg.proj_text_embed.weight.shape) == (32, 768)
    with pytest.raises(NotImplementedError):
        unreg.embed_text(['a'], output_device='cpu')


def test_stub_tokenizer_has_the_call_form_of_the_real_one():
    tok = TR.StubTokenizer(50)
    enc = tok(['a dog barking', 'rain'], return_tensors='pt', padding='longest', max_length=T5.MAX_LENGTH, truncation=True)
    assert enc.input_ids.shape == enc.attention_mask.shape == (2, 4) and enc.input_ids.dtype == torch.long
    assert enc.attention_mask.tolist() == [[1, 1, 1, 1], [1, 1, 0, 0]] and enc.input_ids[1].tolist()[1:] == [1, 0, 0]
    assert int(enc.input_ids.max()) < 50 and tok.calls == 1


def test_install_as_reference_exposes_the_t5_module():
    saved = {k: v for k, v in sys.modules.items() if k == 'audiolm_pytorch' or k.startswith('audiolm_pytorch.')}
    try:
        A.install_as_reference()
        from audiolm_pytorch.t5 import DEFAULT_T5_NAME, get_encoded_dim, t5_encode_text          # reference audiolm_pytorch.py:31
        assert t5_encode_text is A.t5_encode_text and get_encoded_dim is T5.get_encoded_dim and DEFAULT_T5_NAME == 'google/t5-v1_1-base'
        import audiolm_pytorch
        assert audiolm_pytorch.t5 is T5
    finally:
        for k in [k for k in sys.modules if k == 'audiolm_pytorch' or k.startswith('audiolm_pytorch.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_exports():
    for n in ('T5Encoder', 't5_encode_text', 'register_t5', 'load_t5'):
        assert hasattr(A, n)
