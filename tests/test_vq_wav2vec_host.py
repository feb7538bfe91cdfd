"""CPU: the host side of audiolm_pytorch_amd.FairseqVQWav2Vec (loading, the configuration, the key checks, the frame count, the argument contract),
the wiring into install_as_reference(), and the two SoundStream presets.  No kernel runs here."""
import argparse
import inspect
import re

import pytest
import torch

import vq_wav2vec_restated as VR
import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib
from audiolm_pytorch_amd import vq_wav2vec as VQ

TINY_CONV = [(40, 10, 5), (40, 4, 2), (40, 1, 1)]
TINY_ARGS = dict(conv_feature_layers=str(TINY_CONV), log_compression=True, skip_connections_feature_extractor=False, residual_scale=0.5,
                 non_affine_group_norm=False, activation='relu', vq_type='kmeans', vq_groups=2, vq_vars=16, vq_dim=0, combine_groups=False)


def tiny_sd(**kw):
    return VR.random_state_dict(3, conv=TINY_CONV, groups=2, num_vars=16, **kw)


def with_aggregator(sd):
    return {**sd, 'feature_aggregator.conv_layers.0.0.weight': torch.zeros(4, 4, 2), 'wav2vec_predictions.project_to_steps.weight': torch.zeros(4, 4, 1, 2),
            'dropout_feats.p': torch.zeros(1)}


@pytest.mark.parametrize('form', ['args', 'cfg', 'bare'])
def test_checkpoint_forms_load_and_the_aggregator_is_ignored(tmp_path, form):
    sd = with_aggregator(tiny_sd())
    path = tmp_path / f'{form}.pt'
    if form == 'args':
        torch.save({'model': sd, 'args': argparse.Namespace(**TINY_ARGS, arch='wav2vec')}, path)
    elif form == 'cfg':
        torch.save({'model': sd, 'cfg': {'model': dict(TINY_ARGS, _name='wav2vec'), 'task': {}}}, path)
    else:
        torch.save(sd, path)
    if form == 'bare':                                          # no configuration travels with a bare state dict: the released stack does not match
        with pytest.raises(KeyError, match='lacks 15 entries'):
            A.FairseqVQWav2Vec(path)
        m = A.FairseqVQWav2Vec.from_state_dict(torch.load(path, weights_only=True), conv_feature_layers=TINY_CONV)
    else:
        m = A.FairseqVQWav2Vec(path, seq_len_multiple_of=80)
        assert m.seq_len_multiple_of == 80
    assert m.conv_layers == TINY_CONV and m.log_compression and not m.skip_connections and m.affine and not m.combine_groups
    assert m.groups == 2 and m.codebook_size == 16 and m.dim == 40 and m.residual_scale == 0.5 ** 0.5
    kept = {k for k in sd if k.startswith(('feature_extractor.', 'vector_quantizer.'))}
    assert set(dict(m.named_parameters())) == kept == set(m.state_dict())
    for k in kept:
        assert torch.equal(m.state_dict()[k], sd[k])
    m.load_state_dict({k: sd[k] for k in kept})                 # loads by name, strictly
    assert not m.training and not any(p.requires_grad for p in m.parameters())


def test_configuration_is_read_from_the_checkpoint(tmp_path):
    sd = tiny_sd(affine=False, combine_groups=True)
    args = dict(TINY_ARGS, log_compression=False, skip_connections_feature_extractor=True, residual_scale=0.25, non_affine_group_norm=True,
                combine_groups=True)
    torch.save({'model': sd, 'args': argparse.Namespace(**args)}, tmp_path / 'c.pt')
    m = A.FairseqVQWav2Vec(tmp_path / 'c.pt')
    assert not m.log_compression and m.skip_connections and m.residual_scale == 0.5 and not m.affine and m.combine_groups
    assert not any(re.search(r'conv_layers\.\d+\.2\.', k) for k in m.state_dict())


def test_missing_unknown_and_mismatching_entries_raise():
    sd = tiny_sd()
    for drop in ('vector_quantizer.embedding', 'feature_extractor.conv_layers.1.0.weight', 'feature_extractor.conv_layers.2.2.bias'):
        with pytest.raises(KeyError, match='lacks'):
            A.FairseqVQWav2Vec.from_state_dict({k: v for k, v in sd.items() if k != drop}, conv_feature_layers=TINY_CONV)
    with pytest.raises(KeyError, match='unexpected'):
        A.FairseqVQWav2Vec.from_state_dict({**sd, 'encoder.layers.0.fc1.weight': torch.zeros(2)}, conv_feature_layers=TINY_CONV)
    with pytest.raises(KeyError, match='unexpected'):          # non-affine norms have no '.2.' entries
        A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, non_affine_group_norm=True)
    with pytest.raises(ValueError, match='conv layer 1'):
        A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=[(40, 10, 5), (40, 3, 2), (40, 1, 1)])
    for key, bad in (('vq_groups', 4), ('vq_vars', 320), ('combine_groups', True)):
        with pytest.raises(ValueError, match=key):
            A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, **{key: bad})
    with pytest.raises(ValueError, match='embedding'):
        A.FairseqVQWav2Vec.from_state_dict({**sd, 'vector_quantizer.embedding': torch.zeros(16, 2, 10)}, conv_feature_layers=TINY_CONV)
    with pytest.raises(TypeError, match='unknown configuration'):
        A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, offset='auto')


def test_unsupported_options_raise_by_name():
    sd = tiny_sd()
    with pytest.raises(NotImplementedError, match='gumbel'):
        A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, vq_type='gumbel')
    with pytest.raises(NotImplementedError, match='gelu'):
        A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, activation='gelu')
    with pytest.raises(NotImplementedError, match='vq_dim'):
        A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, vq_dim=16)
    A.FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, vq_dim=40)


def test_members_and_defaults_are_the_reference_s():
    sig = inspect.signature(A.FairseqVQWav2Vec.__init__)
    assert list(sig.parameters)[1:] == ['checkpoint_path', 'target_sample_hz', 'seq_len_multiple_of']
    assert [sig.parameters[n].default for n in ('target_sample_hz', 'seq_len_multiple_of')] == [24000, None]
    fsig = inspect.signature(A.FairseqVQWav2Vec.forward)
    assert list(fsig.parameters)[1:] == ['wav_input', 'flatten', 'input_sample_hz']
    assert fsig.parameters['flatten'].default is True and fsig.parameters['input_sample_hz'].default is None
    m = A.FairseqVQWav2Vec.from_state_dict(tiny_sd(), conv_feature_layers=TINY_CONV)
    assert m.target_sample_hz == 24000 and m.seq_len_multiple_of is None and m.downsample_factor == 80
    assert m.groups == 2 and m.codebook_size == 16
    one = A.FairseqVQWav2Vec.from_state_dict(VR.random_state_dict(4, conv=TINY_CONV, groups=1, num_vars=7), conv_feature_layers=TINY_CONV)
    assert one.groups == 1 and one.codebook_size == 7 and not one.combine_groups


def test_released_defaults_without_configuration():
    """a bare released-size state dict needs no configuration: the released conv stack, 2 groups of 320 codes, log compression, affine norms"""
    m = A.FairseqVQWav2Vec.from_state_dict(VR.random_state_dict(1))
    assert m.conv_layers == VR.RELEASED_CONV and m.groups == 2 and m.codebook_size == 320 and m.dim == 512
    assert m.log_compression and not m.skip_connections and m.affine and not m.combine_groups


def test_cpu_tensor_and_bad_rank_raise():
    m = A.FairseqVQWav2Vec.from_state_dict(tiny_sd(), conv_feature_layers=TINY_CONV)
    with pytest.raises(RuntimeError, match='MI355X'):
        m(torch.zeros(1, 800))
    with pytest.raises(RuntimeError, match='MI355X'):
        m.features(torch.zeros(1, 800))


@pytest.mark.parametrize('T', [10, 639, 640, 16000, 16123])
def test_frame_count_is_the_oracle_s_output_length(T):
    sd = VR.random_state_dict(1)
    n = VQ.frame_count(T)
    assert n == VR.frame_count(T)
    if T < 465:                                                  # shorter than the receptive field: no frame, and the oracle's conv stack refuses
        assert n == 0
        with pytest.raises(RuntimeError):
            VR.features(sd, torch.zeros(1, T))
    else:
        assert VR.features(sd, torch.zeros(1, T)).shape == (1, n, 2, 256)
    tiny_n = VQ.frame_count(T, TINY_CONV)
    assert tiny_n == VQ.frame_count(T, str(TINY_CONV)) == VR.frame_count(T, TINY_CONV)
    if T >= 25:                                                  # the tiny stack's receptive field
        assert VR.features(tiny_sd(), torch.zeros(1, T), conv=TINY_CONV).shape[1] == tiny_n
    else:
        assert tiny_n == 0


def test_new_symbols_resolve_in_the_built_library():
    lib = _lib.load()
    for name in ('alm_vqw2v_group_chunks', 'alm_vqw2v_group_stats', 'alm_vqw2v_group_apply', 'alm_vqw2v_group_apply_t', 'alm_vqw2v_conv0_stats',
                 'alm_vqw2v_conv0_apply'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.query('alm_vqw2v_group_chunks', 512, 3199, 1) == -(-512 * 3199 // 4096)
    assert _lib.query('alm_vqw2v_group_chunks', 512, 98, 2) == -(-256 * 98 // 4096)
    assert _lib.query('alm_vqw2v_group_chunks', 512, 98, 3) == -1            # 3 groups do not divide 512 channels
    assert _lib.query('alm_vqw2v_group_chunks', 512, 1 << 22, 1) == -1       # C T = 2^31: an in-group index would not fit 32 bits


def test_install_as_reference_exposes_the_module():
    import sys
    saved = {k: v for k, v in sys.modules.items() if k == 'audiolm_pytorch' or k.startswith('audiolm_pytorch.')}
    try:
        pkg = A.install_as_reference()
        from audiolm_pytorch.vq_wav2vec import FairseqVQWav2Vec
        assert FairseqVQWav2Vec is A.FairseqVQWav2Vec is pkg.FairseqVQWav2Vec
        assert pkg.AudioLMSoundStream is A.AudioLMSoundStream and pkg.MusicLMSoundStream is A.MusicLMSoundStream
    finally:
        for k in [k for k in sys.modules if k == 'audiolm_pytorch' or k.startswith('audiolm_pytorch.')]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize('preset, strides, hz', [('AudioLMSoundStream', (2, 4, 5, 8), 16000), ('MusicLMSoundStream', (3, 4, 5, 8), 24000)])
def test_presets_build_the_reference_s_soundstream(preset, strides, hz):
    make = getattr(A, preset)
    sig = inspect.signature(make)
    assert [(n, p.default) for n, p in sig.parameters.items() if p.kind is not p.VAR_KEYWORD] == [('strides', strides), ('target_sample_hz', hz),
                                                                                                    ('rq_num_quantizers', 12)]
    small = dict(channels=4, codebook_dim=16, codebook_size=32, attn_window_size=8, attn_dim_head=8, attn_heads=2)
    ss = make(**small)
    assert isinstance(ss, A.SoundStream) and ss.target_sample_hz == hz and ss.num_quantizers == 12
    assert ss.seq_len_multiple_of == strides[0] * strides[1] * strides[2] * strides[3]
    direct = A.SoundStream(strides=strides, target_sample_hz=hz, rq_num_quantizers=12, **small)
    assert set(ss.state_dict()) == set(direct.state_dict())
    assert {k: tuple(v.shape) for k, v in ss.state_dict().items()} == {k: tuple(v.shape) for k, v in direct.state_dict().items()}
    assert make(rq_num_quantizers=3, **small).num_quantizers == 3
