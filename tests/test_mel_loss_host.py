"""CPU: the host side of the multi-spectral mel-spectrogram reconstruction loss (audiolm_pytorch_amd/mel_loss.py, csrc/mel_loss.hip, the wiring in
soundstream.py) -- no kernel runs here.  Filterbank and padded window against the float64 restatement (tests/mel_restated.py), buffer names and shapes
against the real reference's (stored in tests/golden/soundstream_losses_mel.pt), the scale table of the default constructor, the C ABI and its
host-side queries, and the refusals that must fire before any launch."""
import os
import re

import pytest
import torch

import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib, ops
from common import GOLDEN_DIR
from mel_restated import MelSpectrogramRestated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False)
SYMBOLS = ('alm_mel_power_fwd', 'alm_mel_project_fwd', 'alm_mel_loss_ws_floats', 'alm_mel_frame_loss_fwd', 'alm_mel_frame_loss_bwd', 'alm_mel_power_bwd')
# (n_fft, win_length, hop_length, n_mels, normalized)
CASES = [(64, 64, 16, 20, False), (128, 32, 8, 64, False), (512, 64, 16, 80, True), (400, None, None, 128, False), (2048, 2048, 512, 64, True),
         (65, 33, 7, 12, True)]


@pytest.fixture(scope='module')
def fixture():
    return torch.load(os.path.join(GOLDEN_DIR, 'soundstream_losses_mel.pt'), weights_only=False)


@pytest.fixture(scope='module')
def with_mel():
    return A.SoundStream(**SMALL, with_discriminators=True, stft_discriminator=True, with_mel_loss=True)       # reference default weight 1e-5


@pytest.mark.parametrize('n_fft,win,hop,n_mels,normalized', CASES)
def test_filterbank_and_padded_window_equal_the_restatement(n_fft, win, hop, n_mels, normalized):
    kw = dict(sample_rate=16000, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, normalized=normalized)
    ours, ref = A.MelSpectrogram(**kw), MelSpectrogramRestated(**kw)
    assert (ours.win_length, ours.hop_length) == (ref.win_length, ref.hop_length)
    assert list(ours.state_dict()) == list(ref.state_dict()) == ['spectrogram.window', 'mel_scale.fb']
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {'spectrogram.window': (ref.win_length,), 'mel_scale.fb': (n_fft // 2 + 1, n_mels)}
    assert all(v.dtype == torch.float32 for v in ours.state_dict().values())
    fb64, w64 = ref.mel_scale.fb, ref.spectrogram.window
    assert fb64.dtype == torch.float64 and torch.equal(ours.mel_scale.fb, fb64.float()) and torch.equal(ours.spectrogram.window, w64.float())
    # the window as the DFT sees it: centred inside n_fft (left pad (n_fft - win_length) // 2, like torch.stft), over sqrt(sum w^2) when normalized
    left = (n_fft - ref.win_length) // 2
    want = torch.zeros(n_fft, dtype=torch.float64)
    want[left:left + ref.win_length] = w64 / w64.pow(2).sum().sqrt() if normalized else w64
    got = ours.padded_window()
    assert got.dtype == torch.float64 and tuple(got.shape) == (n_fft,)
    assert float((got - want).abs().max()) <= 1e-7 and float(got[:left].abs().sum()) == 0. and float(got[left + ref.win_length:].abs().sum()) == 0.
    # frames x basis is the restated spectrogram: the basis holds the window (and the normalisation); rows outside the window's support are zeros
    basis = ours._dft_basis('cpu')
    assert ours._dft_basis('cpu') is basis                       # kept until the buffer changes
    assert float(basis[:left].abs().sum()) == 0. and float(basis[left + ref.win_length:].abs().sum()) == 0.
    x = torch.randn(2, 3 * n_fft, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    frames = torch.nn.functional.pad(x[:, None], (n_fft // 2, n_fft // 2), mode='reflect')[:, 0].unfold(1, n_fft, ref.hop_length)
    X = (frames @ basis.double()).reshape(2, -1, n_fft // 2 + 1, 2)
    mel = (X.pow(2).sum(-1) @ ours.mel_scale.fb.double()).transpose(1, 2)
    want_mel = ref(x)
    assert mel.shape == want_mel.shape and float((mel - want_mel).abs().max()) <= 1e-6 * float(want_mel.abs().max())
    ours.load_state_dict({'spectrogram.window': torch.hamming_window(ref.win_length), 'mel_scale.fb': ours.mel_scale.fb.clone()})
    assert ours._dft_basis('cpu') is not basis                   # a loaded window rebuilds the basis


def test_empty_filters():
    """at n_fft = 64 the 33 bins are 250 Hz apart: 20 of the 64 HTK triangles fall between two bins and are all-zero; none at 512 / 1024 / 2048"""
    zeros = lambda n_fft: int((A.MelSpectrogram(sample_rate=16000, n_fft=n_fft, n_mels=64).mel_scale.fb.abs().sum(0) == 0).sum())
    assert zeros(64) == 20
    assert zeros(512) == zeros(1024) == zeros(2048) == 0


def test_scale_table_and_buffer_names_of_the_default_constructor(fixture, with_mel):
    ts = with_mel.mel_spec_transforms
    assert [t.n_fft for t in ts] == [512, 512, 512, 512, 1024, 2048]
    assert [t.win_length for t in ts] == [64, 128, 256, 512, 1024, 2048]
    assert [t.hop_length for t in ts] == [16, 32, 64, 128, 256, 512]
    assert [t.n_mels for t in ts] == [64] * 6 and all(t.sample_rate == 16000 and not t.normalized for t in ts)
    assert with_mel.mel_spec_recon_alphas == [(w / 2) ** 0.5 for w in (64, 128, 256, 512, 1024, 2048)]
    got = {k: tuple(v.shape) for k, v in with_mel.state_dict().items() if k.startswith('mel_spec_transforms.')}
    assert got == {k: tuple(s) for k, s in fixture['mel_spec_transforms_shapes'].items()} and len(got) == 12
    assert set(with_mel.state_dict()) == set(fixture['shapes']) | set(got)
    assert not {id(p) for p in with_mel.mel_spec_transforms.parameters()}                            # buffers only: nothing for an optimizer
    other = A.SoundStream(**SMALL, with_discriminators=True, stft_discriminator=False, with_mel_loss=True, target_sample_hz=24000, stft_normalized=True,
                          multi_spectral_window_powers_of_two=(5, 9), multi_spectral_n_ffts=(64, 256), multi_spectral_n_mels=(16, 80))
    assert [(t.sample_rate, t.n_fft, t.win_length, t.hop_length, t.n_mels, t.normalized) for t in other.mel_spec_transforms] == \
        [(24000, 64, 32, 8, 16, True), (24000, 512, 512, 128, 80, True)]
    assert other.mel_spec_recon_alphas == [4., 16.]


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\bint\s+(alm_\w+)\s*\(', src))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'mel_loss.hip' in __import__('audiolm_pytorch_amd.build', fromlist=['SOURCES']).SOURCES
    assert hasattr(A, 'MelSpectrogram') and callable(A.multi_spectral_recon_loss)
    for name in ('mel_power', 'mel_project', 'mel_frame_loss', 'mel_frame_loss_bwd', 'mel_power_bwd'):
        assert callable(getattr(ops, name)), name


def test_size_and_envelope_queries_run_on_the_host():
    """the launchers check their arguments before the launch, so outside the envelope they return on a machine without a GPU"""
    assert _lib.query('alm_mel_loss_ws_floats') == 2048
    q = _lib.query
    BAD, UNSUPPORTED = 10001, 10002
    # x, basis, P, X, B, x_from, n, n_fft, hop, F, k_lo, k_hi, stream
    assert q('alm_mel_power_fwd', None, None, None, None, 0, 0, 200, 64, 16, 33, 0, 64, None) == BAD          # no batch
    assert q('alm_mel_power_fwd', None, None, None, None, 2, 3, 200, 64, 16, 33, 0, 64, None) == BAD          # x_from past the batch
    assert q('alm_mel_power_fwd', None, None, None, None, 2, 1, 200, 64, 16, 33, 40, 40, None) == BAD         # empty reduction range
    assert q('alm_mel_power_fwd', None, None, None, None, 2, 1, 200, 64, 16, 33, 0, 65, None) == BAD          # range past n_fft
    assert q('alm_mel_power_fwd', None, None, None, None, 2, 1, 32, 64, 16, 33, 0, 64, None) == UNSUPPORTED   # n <= n_fft / 2: no reflection
    assert q('alm_mel_power_fwd', None, None, None, None, 1 << 20, 1, 1 << 20, 64, 16, 33, 0, 64, None) == UNSUPPORTED       # B T past 2^31
    assert q('alm_mel_project_fwd', None, None, None, 2, 33, 0, 20, None) == BAD
    assert q('alm_mel_project_fwd', None, None, None, 1 << 20, 33, 1 << 12, 20, None) == UNSUPPORTED
    assert q('alm_mel_frame_loss_fwd', None, None, None, None, None, 2, 20, 13, 1.0, None) == BAD            # null outputs
    assert q('alm_mel_frame_loss_bwd', None, None, None, None, 2, 20, 13, 1.0, None) == BAD                  # null upstream gradient
    assert q('alm_mel_frame_loss_bwd', None, None, None, None, 0, 20, 13, 1.0, None) == BAD
    assert q('alm_mel_power_bwd', None, None, None, None, 2, 33, 13, 0, None) == BAD
    assert q('alm_mel_power_bwd', None, None, None, None, 1 << 20, 33, 1 << 12, 20, None) == UNSUPPORTED


def test_refusals_fire_before_any_launch(with_mel):
    with pytest.raises(NotImplementedError, match='MelSpectrogram: power not implemented'):
        A.MelSpectrogram(power=1.)
    with pytest.raises(NotImplementedError, match='MelSpectrogram: f_max, mel_scale not implemented'):
        A.MelSpectrogram(mel_scale='slaney', f_max=4000.)
    with pytest.raises(ValueError, match='win_length'):
        A.MelSpectrogram(n_fft=64, win_length=128)
    t = A.MelSpectrogram(n_fft=64, hop_length=16, n_mels=20)
    with pytest.raises(ValueError, match='too short.*n_fft = 64'):
        t(torch.zeros(1, 32))
    with pytest.raises(RuntimeError, match='MI355X only'):
        t(torch.zeros(1, 200))
    with pytest.raises(ValueError, match='too short.*n_fft = 64'):
        A.multi_spectral_recon_loss(torch.zeros(1, 32), torch.zeros(1, 32), [t], [1.])
    with pytest.raises(ValueError, match='alphas'):
        A.multi_spectral_recon_loss(torch.zeros(1, 200), torch.zeros(1, 200), [t], [1., 2.])
    with pytest.raises(ValueError, match='shape'):
        A.multi_spectral_recon_loss(torch.zeros(1, 200), torch.zeros(2, 200), [t], [1.])
    with pytest.raises(TypeError, match='MelSpectrogramRestated'):
        A.multi_spectral_recon_loss(torch.zeros(1, 200), torch.zeros(1, 200), [MelSpectrogramRestated(n_fft=64)], [1.])
    with pytest.raises(RuntimeError, match='MI355X only'):
        A.multi_spectral_recon_loss(torch.zeros(1, 200), torch.zeros(1, 200), [t], [1.])
    with pytest.raises(ValueError, match='with_discriminators=True'):
        A.SoundStream(**SMALL, with_mel_loss=True)
    with pytest.raises(ValueError, match='multi_spectral_n_ffts'):
        A.SoundStream(**SMALL, with_discriminators=True, with_mel_loss=True, multi_spectral_n_ffts=(512, 1024))
    with pytest.raises(ValueError, match='too short.*n_fft = 2048'):       # 640 samples <= 1024: the 2048-point scale cannot pad, named before the codec runs
        with_mel(torch.zeros(1, 640))
    with pytest.raises(NotImplementedError, match='apply_grad_penalty'):
        with_mel(torch.zeros(1, 1280), apply_grad_penalty=True)


def test_the_switch_gets_past_the_option_checks(with_mel):
    """a with_mel_loss=True model with the reference's default weight has its transforms, and on a CPU tensor both loss branches get past the option
    checks to the refusal of the CPU; without the switch the positive weight still raises by name and nothing is registered"""
    assert with_mel.multi_spectral_recon_loss_weight == 1e-5 and len(with_mel.mel_spec_transforms) == 6
    x = torch.zeros(1, 1280)
    with pytest.raises(RuntimeError, match='MI355X only'):
        with_mel(x)
    with pytest.raises(RuntimeError, match='MI355X only'):
        with_mel(x, return_loss_breakdown=True)
    with pytest.raises(RuntimeError, match='MI355X only'):       # the discriminator branch never touches the mel transforms: no length check either
        with_mel(torch.zeros(1, 640), return_discr_loss=True)
    plain = A.SoundStream(**SMALL, with_discriminators=True, stft_discriminator=True, multi_spectral_n_mels=80)
    assert not hasattr(plain, 'mel_spec_transforms') and not any(k.startswith('mel_spec') for k in plain.state_dict())
    with pytest.raises(NotImplementedError, match='mel-spectrogram'):
        plain(x)
    off = A.SoundStream(**SMALL, with_discriminators=True, stft_discriminator=True, with_mel_loss=True, multi_spectral_recon_loss_weight=0.)
    with pytest.raises(RuntimeError, match='MI355X only'):       # weight 0: the term is off, so a short clip is no reason to refuse
        off(torch.zeros(1, 640))
