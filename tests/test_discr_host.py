"""CPU: the host side of the wave discriminators (audiolm_pytorch_amd/discriminators.py, the opt-in loss branches of soundstream.py) -- no kernel
runs here.  Key names and shapes against the real reference's (stored in tests/golden/soundstream_losses_small.pt), the output-length arithmetic of
every layer and of the pooling, the documented NotImplementedErrors, the opt-in switch, non_discr_parameters() and the C ABI of csrc/discr.hip."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib, ops
from common import GOLDEN_DIR
from discr_restated import MultiScaleDiscriminatorRestated, TinyWaveDiscriminator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False)
SYMBOLS = ('alm_gconv1d_out_len', 'alm_gconv1d_fwd', 'alm_gconv1d_dgrad', 'alm_gconv1d_wgrad_ws_floats', 'alm_gconv1d_wgrad', 'alm_avgpool1d_out_len',
           'alm_avgpool1d_fwd', 'alm_avgpool1d_bwd', 'alm_loss_ws_floats', 'alm_loss_mean_fwd', 'alm_loss_mean_bwd')


@pytest.fixture(scope='module')
def fixture():
    return torch.load(os.path.join(GOLDEN_DIR, 'soundstream_losses_small.pt'), weights_only=False)


@pytest.fixture(scope='module')
def with_discr():
    return A.SoundStream(**SMALL, multi_spectral_recon_loss_weight=0., stft_discriminator=TinyWaveDiscriminator(), with_discriminators=True)


def test_key_names_and_shapes_equal_the_reference(fixture, with_discr):
    want = {k: tuple(s) for k, s in fixture['discriminator_shapes'].items()}
    assert len(want) == 3 * 14
    got = {k: tuple(v.shape) for k, v in with_discr.state_dict().items() if k.startswith('discriminators.')}
    assert got == want
    one = {k: tuple(v.shape) for k, v in A.MultiScaleDiscriminator().state_dict().items()}
    assert one == {k[len('discriminators.0.'):]: s for k, s in want.items() if k.startswith('discriminators.0.')}
    assert set(one) == set(MultiScaleDiscriminatorRestated().state_dict())
    assert sum(p.numel() for p in with_discr.discriminators.parameters()) == sum(math.prod(s) for s in want.values()) == 16_913_859
    assert set(with_discr.state_dict()) == set(fixture['shapes'])                                   # codec + discriminators + the caller's module
    assert isinstance(with_discr.downsamples[0], torch.nn.Identity) and [d.factor for d in with_discr.downsamples[1:]] == [2, 2]
    assert isinstance(with_discr.stft_discriminator, TinyWaveDiscriminator)


@pytest.mark.parametrize('T', [1, 5, 41, 1000, 1283, 2560, 160000])
def test_output_length_arithmetic(T):
    """every layer of the module and the pooling: the C ABI's lengths are torch's"""
    m = MultiScaleDiscriminatorRestated(channels=1, chan_max=1, groups=(1, 1, 1, 1))          # one channel: only the lengths matter
    convs = [m.init_conv, *(layer[0] for layer in m.conv_layers), m.final_conv[0], m.final_conv[2]]
    x = torch.zeros(1, 1, T)
    n = T
    for conv in convs:
        x = conv(x)
        n = ops.gconv1d_out_len(n, conv.kernel_size[0], conv.stride[0], conv.padding[0])
        assert n == x.shape[-1]
    assert ops.gconv1d_out_len(5, 41, 4, 20) == 2 and ops.gconv1d_out_len(5, 41, 4, 17) == -1       # padded input shorter than the kernel
    for f in (1, 2, 3, 4):
        assert ops.avgpool1d_out_len(T, f) == F.avg_pool1d(torch.zeros(1, 1, T), 2 * f, stride=f, padding=f).shape[-1]


def test_weight_gradient_workspace_query():
    """splits x (numel(dW) + Cout) floats, a function of the shapes alone; -1 outside the envelope"""
    q = lambda *a: _lib.query('alm_gconv1d_wgrad_ws_floats', *a)
    for B, Cin, Cout, T, k, s, p, g in ((2, 16, 64, 301, 41, 4, 20, 4), (2, 1024, 1024, 3, 5, 1, 2, 1), (16, 1, 16, 160000, 15, 1, 7, 1)):
        n = q(B, Cin, Cout, T, k, s, p, g)
        slab = Cout * (Cin // g) * k + Cout
        assert n > 0 and n % slab == 0 and 1 <= n // slab <= 512 and n == q(B, Cin, Cout, T, k, s, p, g)
    assert q(2, 16, 64, 301, 41, 4, 20, 3) == -1                 # channels not divisible by the groups
    assert q(1, 4, 4, 5, 41, 4, 0, 1) == -1                      # no output step
    assert _lib.query('alm_loss_ws_floats') >= 1024


def test_documented_refusals(with_discr):
    x = torch.zeros(1, 640)
    mel = A.SoundStream(**SMALL, stft_discriminator=TinyWaveDiscriminator(), with_discriminators=True)     # reference default weight 1e-5
    with pytest.raises(NotImplementedError, match='mel-spectrogram'):
        mel(x)
    with pytest.raises(NotImplementedError, match='mel-spectrogram'):
        mel(x, return_discr_loss=True)
    with pytest.raises(NotImplementedError, match='apply_grad_penalty'):
        with_discr(x, return_discr_loss=True, apply_grad_penalty=True)
    no_stft = A.SoundStream(**SMALL, multi_spectral_recon_loss_weight=0., with_discriminators=True)
    assert not hasattr(no_stft, 'stft_discriminator')
    for kw in (dict(), dict(return_discr_loss=True), dict(return_loss_breakdown=True)):
        with pytest.raises(NotImplementedError, match='ComplexSTFTDiscriminator'):
            no_stft(x, **kw)
    with pytest.raises(NotImplementedError, match='is_denoising'):
        with_discr(x, target=x, is_denoising=True)
    with pytest.raises(TypeError, match='stft_discriminator'):
        A.SoundStream(**SMALL, stft_discriminator='complex', with_discriminators=True)
    with pytest.raises(RuntimeError, match='MI355X only'):       # past the option checks the CPU is refused, as everywhere
        with_discr(x, return_discr_loss=True)


def test_without_the_switch_nothing_is_registered():
    plain = A.SoundStream(**SMALL)
    passed = A.SoundStream(**SMALL, stft_discriminator=TinyWaveDiscriminator(), discr_multi_scales=(1, 0.5), feature_loss_weight=3)
    for ss in (plain, passed):
        assert all(k.startswith(('encoder.', 'decoder.', 'rq.')) for k in ss.state_dict())
        assert not any(hasattr(ss, n) for n in ('discriminators', 'downsamples', 'stft_discriminator'))
        assert [n for n, _ in ss.named_children()] == ['encoder', 'decoder', 'rq']
        x = torch.zeros(1, 640)
        for kw in (dict(), dict(return_discr_loss=True), dict(return_discr_losses_separately=True), dict(return_loss_breakdown=True),
                   dict(apply_grad_penalty=True, return_recons_only=True), dict(return_recons_only=True, target=x)):
            with pytest.raises(NotImplementedError, match='with_discriminators=True'):
                ss(x, **kw)
    default = A.SoundStream(codebook_size=1024)                  # the reference defaults: LocalTransformer on both sides
    assert sorted({k.split('.')[0] for k in default.state_dict()}) == ['decoder', 'decoder_attn', 'encoder', 'encoder_attn', 'rq']
    assert len(plain.non_discr_parameters()) == len(list(plain.parameters()))


def test_non_discr_parameters_excludes_exactly_the_discriminators(with_discr):
    rest = {id(p) for p in with_discr.non_discr_parameters()}
    discr = {id(p) for p in with_discr.discriminators.parameters()} | {id(p) for p in with_discr.stft_discriminator.parameters()}
    every = {id(p) for p in with_discr.parameters()}
    assert rest | discr == every and not rest & discr
    assert len(rest) == len(with_discr.non_discr_parameters())                                      # no parameter twice
    attn = A.SoundStream(codebook_size=32, stft_discriminator=False, with_discriminators=True)
    names = {id(p): n for n, p in attn.named_parameters()}
    kept = {names[id(p)].split('.')[0] for p in attn.non_discr_parameters()}
    assert kept == {'encoder', 'decoder', 'encoder_attn', 'decoder_attn'}
    assert {names[i].split('.')[0] for i in names if i not in {id(p) for p in attn.non_discr_parameters()}} == {'discriminators'}


def test_symbols_are_declared_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\bint\s+(alm_\w+)\s*\(', src))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'discr.hip' in __import__('audiolm_pytorch_amd.build', fromlist=['SOURCES']).SOURCES
    for name in ('MultiScaleDiscriminator',):
        assert hasattr(A, name)
