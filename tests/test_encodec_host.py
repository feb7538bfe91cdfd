"""CPU: the host side of audiolm_pytorch_amd.EncodecWrapper and the restated EnCodec (tests/encodec_restated.py) it is checked against on the GPU.

The restatement is pinned in fp64 to the values transformers' EncodecModel computed for the tiny configuration (tests/golden/encodec_tiny.pt, written by
tests/golden/make_encodec_golden.py), and directly to transformers at the same configuration where it is installed.  Loading, the key maps, the
bandwidth table and the argument contract need no GPU.  No kernel runs here."""
import os

import pytest
import torch

import encodec_restated as ER
import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import encodec as ENC
from common import GOLDEN_DIR


def tiny():
    return torch.load(os.path.join(GOLDEN_DIR, 'encodec_tiny.pt'), weights_only=True)


def tiny_module(t=None, **kw):
    t = t or tiny()
    return A.EncodecWrapper.from_state_dict(t['state_dict'], strides=(2, 4), bandwidth=t['bandwidth'], **dict(t['config'], **kw))


def test_restatement_matches_committed_transformers_values():
    t = tiny()
    sd, cfg = t['state_dict'], t['config']
    assert set(t['waves']) == {'even', 'ragged'}
    for name, wave in t['waves'].items():
        want = t['hf'][name]
        f = ER.encoder(sd, wave, torch.float64, **cfg)
        n = -(-wave.shape[1] // 8)
        assert f.shape == want['features64'].shape == (2, n, 16) and f.dtype == torch.float64
        assert float((f - want['features64']).abs().max()) <= 1e-10
        c = ER.codes(sd, f, 4)
        assert c.dtype == torch.long and torch.equal(c, want['codes'])
        y = ER.decode(sd, c, torch.float64, **cfg)
        assert y.shape == want['decoded64'].shape == (2, 1, n * 8)
        assert float((y - want['decoded64']).abs().max()) <= 1e-10


def test_restatement_matches_transformers_directly():
    pytest.importorskip('transformers')
    from make_encodec_golden import BANDWIDTH, TINY, hf_model
    sd = ER.random_state_dict(5, num_codebooks=4, **TINY)
    wave = torch.randn(3, 8 * 31 + 5, generator=torch.Generator().manual_seed(6)) * 0.3
    model = hf_model(sd, TINY)
    with torch.no_grad():
        feats = model.encoder(wave.double()[:, None])
        codes = model.quantizer.encode(feats, BANDWIDTH)
        audio = model.decoder(model.quantizer.decode(codes))
    f = ER.encoder(sd, wave, torch.float64, **TINY)
    assert float((f - feats.transpose(1, 2)).abs().max()) <= 1e-10
    assert torch.equal(ER.codes(sd, f, 4), codes.permute(1, 2, 0))
    assert float((ER.decode(sd, codes.permute(1, 2, 0), torch.float64, **TINY) - audio).abs().max()) <= 1e-10


def test_recorded_reference_forward_matches_the_restatement():
    """what the reference's own forward / get_emb_from_indices / decode_from_codebook_indices returned = the restated pieces in the same order"""
    t = tiny()
    sd, cfg = t['state_dict'], t['config']
    rec = torch.load(os.path.join(GOLDEN_DIR, 'encodec_ref_forward.pt'), weights_only=True)
    f = ER.encoder(sd, rec['wave3'], torch.float64, **cfg)
    c = ER.codes(sd, f, 4)
    assert rec['encoded']['codes'].shape == (3, 26, 4) and torch.equal(c, rec['encoded']['codes']) and torch.equal(c, rec['codes_only'])
    assert float((ER.emb(sd, c) - rec['encoded']['emb']).abs().max()) <= 1e-12
    assert torch.equal(rec['get_emb_from_indices'], rec['encoded']['emb'])
    c23 = ER.codes(sd, ER.encoder(sd, rec['wave23'].reshape(6, -1), torch.float64, **cfg), 4)
    assert rec['lead_dims']['codes'].shape == (2, 3, 12, 4) and torch.equal(c23.view(2, 3, 12, 4), rec['lead_dims']['codes'])
    assert rec['lead_dims']['emb'].shape == (2, 3, 12, 16)
    y = ER.decode(sd, c[:1], torch.float64, **cfg)
    assert rec['decode_b1'].shape == (1, 1, 208)
    assert float((y - rec['decode_b1']).abs().max()) <= 1e-12          # b = 1: the overlap-add multiplies and divides by the same window
    assert float((y - rec['decode_emb']).abs().max()) <= 1e-12
    assert rec['seq_len_multiple_of'] == 8


def test_key_maps_round_trip():
    sd = tiny()['state_dict']
    meta = ENC.hf_to_meta_state_dict(sd, upsampling_ratios=(4, 2))
    assert 'encoder.model.0.conv.conv.bias' in meta and 'quantizer.vq.layers.0._codebook.embed' in meta
    assert any(k.startswith('decoder.model.3.convtr.convtr.') for k in meta) and any(k.startswith('decoder.model.4.shortcut.conv.conv.') for k in meta)
    assert any(k.startswith('encoder.model.7.lstm.weight_ih_l1') for k in meta)
    back = ENC.meta_to_hf_state_dict(meta)
    assert list(back) == list(sd) and all(back[k] is sd[k] for k in sd)
    assert ENC.hf_to_meta_state_dict(back, upsampling_ratios=(4, 2)).keys() == meta.keys()
    with pytest.raises(KeyError):
        ENC.meta_to_hf_state_dict({'something.else': torch.zeros(1)})
    with pytest.raises(KeyError):
        ENC.hf_to_meta_state_dict({'something.else': torch.zeros(1)})


def test_both_weight_norm_spellings_load_and_buffers_are_ignored():
    t = tiny()
    sd = t['state_dict']
    old = {k.replace('.parametrizations.weight.original0', '.weight_g').replace('.parametrizations.weight.original1', '.weight_v'): v for k, v in sd.items()}
    assert old.keys() != sd.keys()
    for q in range(4):
        old[f'quantizer.layers.{q}.codebook.inited'] = torch.tensor([True])
        old[f'quantizer.layers.{q}.codebook.cluster_size'] = torch.zeros(32)
        old[f'quantizer.layers.{q}.codebook.embed_avg'] = torch.zeros(32, 16)
    a, b = tiny_module(t), A.EncodecWrapper.from_state_dict(old, strides=(2, 4), bandwidth=t['bandwidth'], **t['config'])
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert 'encoder.layers.0.conv.weight_g' in sa and 'encoder.layers.7.lstm.weight_ih_l0' in sa and 'quantizer.layers.3.codebook.embed' in sa
    assert not [k for k in sa if 'inited' in k or 'cluster_size' in k or 'embed_avg' in k]
    with pytest.raises(KeyError):
        A.EncodecWrapper.from_state_dict({k: v for k, v in sd.items() if k != 'decoder.layers.0.conv.bias'}, strides=(2, 4), bandwidth=60., **t['config'])
    with pytest.raises(KeyError):
        A.EncodecWrapper.from_state_dict(dict(sd, stray=torch.zeros(1)), strides=(2, 4), bandwidth=60., **t['config'])
    with pytest.raises(ValueError):
        A.EncodecWrapper.from_state_dict(sd, strides=(2, 4), bandwidth=60., **dict(t['config'], num_filters=8))


def test_members_and_the_bandwidth_table(tmp_path):
    t = tiny()
    m = tiny_module(t)
    assert (m.target_sample_hz, m.codebook_dim, m.rq_groups, m.num_quantizers, m.strides) == (24000, 16, 1, 4, (2, 4))
    assert m.seq_len_multiple_of == m.downsample_factor == 8 and not m.training
    full = {k: torch.zeros(s) for k, s in ER._shapes(ER.config()).items()}
    full.update({f'quantizer.layers.{q}.codebook.embed': torch.zeros(1024, 128) for q in range(32)})
    for bw, q in ((1.5, 2), (3.0, 4), (6.0, 8), (12.0, 16), (24.0, 32)):
        m = A.EncodecWrapper.from_state_dict(full, bandwidth=bw)
        assert m.num_quantizers == q and ER.num_quantizers(bw, ER.config()) == q
    assert (m.codebook_dim, m.seq_len_multiple_of, m.strides) == (128, 320, (2, 4, 5, 8))
    assert sum(p.numel() for p in m.parameters()) + 32 * 1024 * 128 == sum(v.numel() for v in full.values())
    with pytest.raises(KeyError):                                                  # 24 kbps needs 32 codebooks
        A.EncodecWrapper.from_state_dict({k: v for k, v in full.items() if not k.startswith('quantizer.layers.31.')}, bandwidth=24.0)
    path = tmp_path / 'encodec.pt'
    torch.save(t['state_dict'], path)
    m2 = A.EncodecWrapper(24000, (2, 4), 8, t['bandwidth'], checkpoint_path=str(path), **t['config'])
    assert m2.num_quantizers == 4 and all(torch.equal(v, tiny_module(t).state_dict()[k]) for k, v in m2.state_dict().items())


def test_construction_without_local_weights_raises():
    with pytest.raises(NotImplementedError, match='[Hh]ub names are never resolved'):
        A.EncodecWrapper()
    with pytest.raises(NotImplementedError, match='never resolved'):
        A.EncodecWrapper(24000, (2, 4, 5, 8), 8, 6.0)
    with pytest.raises(FileNotFoundError):
        A.EncodecWrapper(checkpoint_path='/nonexistent/encodec_24khz.pt')


@pytest.mark.parametrize('key, value', [('norm_type', 'time_group_norm'), ('use_causal_conv', False), ('normalize', True), ('chunk_length_s', 1.0),
                                        ('audio_channels', 2), ('trim_right_ratio', 0.5), ('pad_mode', 'constant'), ('num_lstm_layers', 3)])
def test_everything_outside_the_causal_mono_model_raises_by_name(key, value):
    t = tiny()
    with pytest.raises(NotImplementedError, match=key):
        tiny_module(t, **{key: value})


def test_argument_contract():
    t = tiny()
    with pytest.raises(AssertionError):
        A.EncodecWrapper.from_state_dict(t['state_dict'], target_sample_hz=48000, strides=(2, 4), bandwidth=60., **t['config'])
    with pytest.raises(ValueError):
        A.EncodecWrapper.from_state_dict(t['state_dict'], strides=(2, 4, 5, 8), bandwidth=60., **t['config'])
    with pytest.raises(TypeError):
        tiny_module(t, no_such_option=1)
    m = tiny_module(t)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 320))
    with pytest.raises(RuntimeError):
        m.decode_from_codebook_indices(torch.zeros(1, 8, 4, dtype=torch.long))
    with pytest.raises(RuntimeError):
        m.get_emb_from_indices(torch.zeros(1, 8, 4, dtype=torch.long))
    with pytest.raises(RuntimeError):
        m.decode(torch.zeros(1, 8, 16))


def test_install_as_reference_exposes_the_encodec_module():
    import sys
    saved = {k: v for k, v in sys.modules.items() if k == 'audiolm_pytorch' or k.startswith('audiolm_pytorch.')}
    try:
        pkg = A.install_as_reference()
        from audiolm_pytorch.encodec import EncodecWrapper
        assert EncodecWrapper is A.EncodecWrapper is pkg.EncodecWrapper
    finally:
        for k in [k for k in sys.modules if k == 'audiolm_pytorch' or k.startswith('audiolm_pytorch.')]:
            del sys.modules[k]
        sys.modules.update(saved)
