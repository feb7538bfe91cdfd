"""CPU: the host side of audiolm_pytorch_amd.HubertWithKmeans and the restated HuBERT (tests/hubert_restated.py) it is checked against on the GPU.

The restatement is pinned in fp64 to transformers.HubertModel (an independent implementation of the same architecture) at base width, and to a
committed fixture of HF features where transformers is absent; a second fixture holds ids recorded from the reference's own
HubertWithKmeans.forward.  Loading, the key map, the frame count and the argument contract need no GPU.  No kernel runs here."""
import os

import pytest
import torch

import hubert_restated as HR
import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib
from audiolm_pytorch_amd import hubert_kmeans as HK
from common import GOLDEN_DIR


def tiny():
    return torch.load(os.path.join(GOLDEN_DIR, 'hubert_tiny.pt'), weights_only=True)


def tiny_module(**kw):
    t = tiny()
    c = t['config']
    return A.HubertWithKmeans.from_state_dict(t['state_dict'], t['centres'], output_layer=c['layers'], conv_feature_layers=c['conv'],
                                              encoder_attention_heads=c['heads'], conv_pos_groups=c['groups'], **kw), t


def test_restatement_matches_hf_hubert_base_fp64():
    """base width, 9 layers, seeded weights, 2 x 2 s: the same fp64 arithmetic up to summation order -> 1e-9 absolute"""
    pytest.importorskip('transformers')
    from make_hubert_golden import hf_model
    sd = HR.random_state_dict(1, layers=9)
    wave = torch.randn(2, 32000, generator=torch.Generator().manual_seed(2)) * 0.3
    model = hf_model(sd, 9, 12, 3072, HR.BASE_CONV, 128, 16)
    with torch.no_grad():
        want = model(wave.double()).last_hidden_state
    got = HR.features(sd, wave, 9, dtype=torch.float64)
    assert got.shape == want.shape == (2, 99, 768)
    err = float((got - want).abs().max())
    print('restatement vs HF fp64: max abs', err)
    assert err <= 1e-9


def test_restatement_matches_committed_hf_features():
    t = tiny()
    c = t['config']
    got = HR.features(t['state_dict'], t['wave'], c['layers'], c['heads'], c['conv'], c['groups'], torch.float64)
    assert got.shape == t['hf_features64'].shape
    assert float((got - t['hf_features64']).abs().max()) <= 1e-9


def test_recorded_reference_forward_matches_restated_assignment():
    """the ids the reference's forward recorded = curtail, restated model, nearest centre (first index), (b, n) for both values of flatten"""
    t = tiny()
    c = t['config']
    rec = torch.load(os.path.join(GOLDEN_DIR, 'hubert_ref_forward.pt'), weights_only=True)
    assert {(k['seq_len_multiple_of'], k['flatten']) for k in rec['cases']} == {(None, True), (None, False), (320, True), (320, False)}
    for case in rec['cases']:
        wave, mult = rec['wave'], case['seq_len_multiple_of']
        if mult is not None:
            wave = wave[..., :wave.shape[-1] // mult * mult]
        f = HR.features(t['state_dict'], wave, c['layers'], c['heads'], c['conv'], c['groups'], torch.float64)
        ids = HR.distances(f, t['centres']).argmin(-1)
        assert case['ids'].dtype == torch.long and case['ids'].shape == (wave.shape[0], HR.frame_count(wave.shape[-1], c['conv']))
        assert torch.equal(case['ids'], ids)


@pytest.mark.parametrize('T', [400, 719, 720, 16000, 32000, 160000, 480000, 5003])
def test_frame_count(T):
    assert HK.frame_count(T) == (T - 400) // 320 + 1 == HR.frame_count(T)


def test_members_and_defaults():
    import inspect
    sig = inspect.signature(A.HubertWithKmeans.__init__)
    assert list(sig.parameters)[1:] == ['checkpoint_path', 'kmeans_path', 'target_sample_hz', 'seq_len_multiple_of', 'output_layer']
    assert [sig.parameters[n].default for n in ('target_sample_hz', 'seq_len_multiple_of', 'output_layer')] == [16000, None, 9]
    fsig = inspect.signature(A.HubertWithKmeans.forward)
    assert list(fsig.parameters)[1:4] == ['wav_input', 'flatten', 'input_sample_hz']
    assert fsig.parameters['flatten'].default is True and fsig.parameters['input_sample_hz'].default is None
    m, t = tiny_module(seq_len_multiple_of=320)
    assert m.groups == 1 and m.codebook_size == 50 and m.downsample_factor == 320
    assert m.target_sample_hz == 16000 and m.seq_len_multiple_of == 320 and m.output_layer == 2
    assert m.cluster_centers.shape == (50, 64) and 'cluster_centers' in dict(m.named_buffers())
    assert not m.training and not any(p.requires_grad for p in m.parameters())


def test_parameters_carry_fairseq_names_and_extra_layers_are_dropped():
    sd = HR.random_state_dict(3, dim=64, layers=2, ffn=128, conv=tiny()['config']['conv'], conv_pos=32, extra_layers=1)
    sd['mask_emb'] = torch.zeros(64)
    sd['final_proj.weight'] = torch.zeros(8, 64)
    sd['final_proj.bias'] = torch.zeros(8)
    sd['label_embs_concat'] = torch.zeros(10, 8)
    m = A.HubertWithKmeans.from_state_dict(sd, torch.zeros(5, 64), output_layer=2, conv_feature_layers=tiny()['config']['conv'], encoder_attention_heads=1)
    names = set(dict(m.named_parameters()))
    kept = {k for k in sd if not k.startswith(('mask_emb', 'final_proj', 'label_embs')) and not k.startswith('encoder.layers.2.')}
    assert names == kept
    assert set(m.state_dict()) == kept | {'cluster_centers'}
    for k in kept:
        assert torch.equal(m.state_dict()[k], sd[k])
    m.load_state_dict({**{k: sd[k] for k in kept}, 'cluster_centers': torch.ones(5, 64)})          # loads by name, strictly


def test_weight_norm_is_folded_once_at_load():
    m, t = tiny_module()
    g, v = t['state_dict']['encoder.pos_conv.0.weight_g'].double(), t['state_dict']['encoder.pos_conv.0.weight_v'].double()
    w = v * g / v.pow(2).sum((0, 1), keepdim=True).sqrt()
    assert float((m._pos_w.double() - w).abs().max()) <= 1e-6 * float(w.abs().max())
    assert '_pos_w' not in m.state_dict()


def test_missing_key_fails_loudly():
    t = tiny()
    sd = dict(t['state_dict'])
    del sd['encoder.layers.1.fc2.bias']
    with pytest.raises(KeyError, match='encoder.layers.1.fc2.bias'):
        A.HubertWithKmeans.from_state_dict(sd, t['centres'], output_layer=2, conv_feature_layers=t['config']['conv'], encoder_attention_heads=1)
    with pytest.raises(KeyError):                       # asking for more layers than the checkpoint has
        A.HubertWithKmeans.from_state_dict(t['state_dict'], t['centres'], output_layer=3, conv_feature_layers=t['config']['conv'],
                                           encoder_attention_heads=1)


@pytest.mark.parametrize('option, match', [(dict(layer_norm_first=True), 'layer_norm_first'), (dict(extractor_mode='layer_norm'), 'extractor_mode'),
                                           (dict(normalize=True), 'normalize'), (dict(conv_bias=True), 'conv_bias')])
def test_unsupported_options_raise(option, match):
    with pytest.raises(NotImplementedError, match=match):
        tiny_module(**option)


def test_padding_mask_and_cpu_input_raise():
    m, t = tiny_module()
    with pytest.raises(NotImplementedError, match='padding_mask'):
        m(t['wave'], padding_mask=torch.zeros(2, 4000, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='runs on the MI355X only'):
        m(t['wave'])
    with pytest.raises(NotImplementedError, match='head width'):
        tiny_module_heads2()


def tiny_module_heads2():
    t = tiny()
    c = t['config']
    return A.HubertWithKmeans.from_state_dict(t['state_dict'], t['centres'], output_layer=2, conv_feature_layers=c['conv'], encoder_attention_heads=2)


def test_loads_fairseq_layout_checkpoint_and_joblib_kmeans(tmp_path):
    sklearn_cluster = pytest.importorskip('sklearn.cluster')
    joblib = pytest.importorskip('joblib')
    import numpy as np
    t = tiny()
    c = t['config']
    sd = dict(t['state_dict'])
    sd['mask_emb'] = torch.zeros(64)
    sd['final_proj.weight'] = torch.zeros(8, 64)
    sd['final_proj.bias'] = torch.zeros(8)
    sd['label_embs_concat'] = torch.zeros(10, 8)
    conv_str = '[(32,10,5)] + [(32,3,2)] * 4 + [(32,2,2)] * 2'
    model_cfg = {'_name': 'hubert', 'conv_feature_layers': conv_str, 'encoder_attention_heads': 1, 'encoder_layers': 2, 'layer_norm_first': False,
                 'extractor_mode': 'default', 'conv_bias': False, 'conv_pos': 32, 'conv_pos_groups': 16}
    ckpt = tmp_path / 'hubert.pt'
    torch.save({'model': sd, 'cfg': {'model': model_cfg, 'task': {'normalize': False}}, 'args': None}, ckpt)
    km = sklearn_cluster.MiniBatchKMeans(n_clusters=50, n_init=1)
    km.cluster_centers_ = t['centres'].numpy().astype(np.float32)
    kpath = tmp_path / 'km.bin'
    joblib.dump(km, kpath)
    m = A.HubertWithKmeans(str(ckpt), str(kpath), output_layer=2)
    assert m.conv_layers == [tuple(l) for l in c['conv']] and m.heads == 1 and m.dim == 64 and m.codebook_size == 50
    assert torch.equal(m.cluster_centers, t['centres'])
    for k, v in m.state_dict().items():
        if k != 'cluster_centers':
            assert torch.equal(v, sd[k]), k
    # .pt / .npy centres, a bare state dict, and an old-style `args` namespace
    torch.save(t['centres'], tmp_path / 'c.pt')
    np.save(tmp_path / 'c.npy', t['centres'].numpy())
    import argparse
    torch.save({'model': sd, 'args': argparse.Namespace(**model_cfg, normalize=False)}, tmp_path / 'old.pt')
    for ck, kp in ((tmp_path / 'old.pt', tmp_path / 'c.pt'), (tmp_path / 'old.pt', tmp_path / 'c.npy')):
        m2 = A.HubertWithKmeans(ck, kp, output_layer=2)
        assert torch.equal(m2.cluster_centers, t['centres']) and m2.conv_layers == m.conv_layers
    torch.save({'model': sd, 'cfg': {'model': dict(model_cfg, layer_norm_first=True), 'task': {'normalize': False}}}, tmp_path / 'large.pt')
    with pytest.raises(NotImplementedError, match='layer_norm_first'):
        A.HubertWithKmeans(tmp_path / 'large.pt', tmp_path / 'c.pt', output_layer=2)
    torch.save({'model': sd, 'cfg': {'model': model_cfg, 'task': {'normalize': True}}}, tmp_path / 'norm.pt')
    with pytest.raises(NotImplementedError, match='normalize'):
        A.HubertWithKmeans(tmp_path / 'norm.pt', tmp_path / 'c.pt', output_layer=2)
    with pytest.raises(AssertionError, match='does not exist'):
        A.HubertWithKmeans(tmp_path / 'nowhere.pt', tmp_path / 'c.pt')


def test_hf_key_map_round_trips():
    sd = HR.random_state_dict(4, dim=64, layers=2, ffn=128, conv=tiny()['config']['conv'], conv_pos=32)
    sd['mask_emb'] = torch.zeros(64)
    hf = HK.fairseq_to_hf_state_dict(sd)
    assert 'encoder.layers.1.feed_forward.output_dense.weight' in hf and 'feature_projection.projection.bias' in hf and 'masked_spec_embed' in hf
    back = HK.hf_to_fairseq_state_dict({'hubert.' + k: v for k, v in hf.items()})
    assert set(back) == set(sd) and all(back[k] is sd[k] for k in sd)
    hf['encoder.pos_conv_embed.conv.parametrizations.weight.original0'] = hf.pop('encoder.pos_conv_embed.conv.weight_g')
    hf['encoder.pos_conv_embed.conv.parametrizations.weight.original1'] = hf.pop('encoder.pos_conv_embed.conv.weight_v')
    back = HK.hf_to_fairseq_state_dict(hf)
    assert set(back) == set(sd) and all(back[k] is sd[k] for k in sd)
    with pytest.raises(KeyError):
        HK.hf_to_fairseq_state_dict({'lm_head.weight': torch.zeros(1)})


def test_hf_model_state_dict_maps_onto_the_module():
    transformers = pytest.importorskip('transformers')
    from make_hubert_golden import hf_model
    t = tiny()
    c = t['config']
    model = hf_model(t['state_dict'], c['layers'], c['heads'], c['ffn'], c['conv'], c['conv_pos'], c['groups'], dtype=torch.float32)
    sd = HK.hf_to_fairseq_state_dict(model.state_dict())
    m = A.HubertWithKmeans.from_state_dict(sd, t['centres'], output_layer=2, conv_feature_layers=c['conv'], encoder_attention_heads=1)
    for k, v in m.state_dict().items():
        if k != 'cluster_centers':
            assert torch.equal(v, t['state_dict'][k]), k


def test_new_entry_points_are_bound():
    for name in ('alm_hubert_conv0_chunks', 'alm_hubert_conv0_stats', 'alm_hubert_conv0_apply', 'alm_conv1d_valid', 'alm_layernorm_bct_split', 'alm_mha_attn_fwd'):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.query('alm_hubert_conv0_chunks', 96000) == 94 and _lib.query('alm_hubert_conv0_chunks', 1) == 1


def test_exported_and_free_of_fairseq_and_test_imports():
    import re
    assert A.HubertWithKmeans is HK.HubertWithKmeans
    src = open(HK.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+(fairseq|hubert_restated|torchaudio|transformers)\b', src, flags=re.M)
