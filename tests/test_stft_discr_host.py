"""CPU: the host side of the native ComplexSTFTDiscriminator (audiolm_pytorch_amd/discriminators.py, csrc/stft_discr.hip, the wiring in
soundstream.py) -- no kernel runs here.  Key names, shapes and seeded initial values against the real reference's (stored in
tests/golden/soundstream_losses_stft.pt), the C ABI, the shape and workspace queries against torch's own output shapes, the SoundStream keywords,
and the refusals that must fire before any launch."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib, ops
from common import GOLDEN_DIR
from stft_discr_restated import ComplexSTFTDiscriminatorRestated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SS = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False, multi_spectral_recon_loss_weight=0.)
SMALL = dict(channels=4, strides=((1, 2), (2, 2)), chan_mults=(1, 2), n_fft=64, hop_length=16, win_length=64)
SYMBOLS = ('alm_stft_frames', 'alm_stft_fwd', 'alm_stft_bwd_ws_floats', 'alm_stft_bwd', 'alm_cconv2d_out_hw', 'alm_cconv2d_fwd', 'alm_cconv2d_dgrad',
           'alm_cconv2d_wgrad_ws_floats', 'alm_cconv2d_wgrad', 'alm_modrelu_ws_floats', 'alm_modrelu_fwd', 'alm_modrelu_bwd', 'alm_cabs_fwd', 'alm_cabs_bwd')
STFT_CASES = [(2, 2560, 1024, 256, 1024, False), (1, 513, 1024, 256, 1024, False), (3, 331, 64, 16, 48, False), (2, 100, 32, 5, 32, True)]
CCONV_CASES = [(2, 1, 32, 37, 11, 7, 7, 1, 1, 3, 3), (2, 32, 32, 19, 6, 3, 3, 1, 1, 1, 1), (2, 32, 64, 19, 6, 3, 4, 1, 2, 1, 2),
               (2, 64, 128, 19, 4, 4, 4, 2, 2, 2, 2), (2, 256, 256, 9, 2, 3, 3, 1, 1, 1, 1), (1, 256, 256, 9, 1, 4, 4, 2, 2, 2, 2),
               (2, 256, 1, 65, 2, 16, 1, 1, 1, 0, 0), (2, 4, 8, 33, 21, 3, 4, 1, 2, 1, 2), (1, 8, 1, 17, 6, 16, 1, 1, 1, 0, 0)]


@pytest.fixture(scope='module')
def fixture():
    return torch.load(os.path.join(GOLDEN_DIR, 'soundstream_losses_stft.pt'), weights_only=False)


def test_key_names_shapes_and_seeded_values_equal_the_reference(fixture):
    want = {k[len('stft_discriminator.'):]: tuple(s) for k, s in fixture['stft_discriminator_shapes'].items()}
    assert len(want) == 2 + 6 * 7 + 2
    torch.manual_seed(0)
    ours = A.ComplexSTFTDiscriminator()
    sd = ours.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd) == list(ComplexSTFTDiscriminatorRestated().state_dict())
    sums = fixture['init_sums']                                  # the same CPU construction in the same order: the same values
    assert set(sums) == set(sd)
    for k, v in sd.items():
        assert float(v.double().sum()) == pytest.approx(sums[k], rel=1e-12, abs=1e-12), k
    assert all(p.dtype == torch.float32 for p in ours.parameters())


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\bint\s+(alm_\w+)\s*\(', src))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r'#define\s+ALM_LOSS_L1_COMPLEX\s+4\b', src) and ops.LOSS_L1_COMPLEX == 4
    assert 'stft_discr.hip' in __import__('audiolm_pytorch_amd.build', fromlist=['SOURCES']).SOURCES
    assert hasattr(A, 'ComplexSTFTDiscriminator')
    for name in ('stft', 'stft_bwd', 'cconv2d', 'cconv2d_dgrad', 'cconv2d_wgrad', 'modrelu', 'modrelu_bwd', 'complex_abs', 'complex_abs_bwd'):
        assert callable(getattr(ops, name)), name


@pytest.mark.parametrize('B,n,n_fft,hop,win,normalized', STFT_CASES)
def test_stft_frames_and_basis_agree_with_torch(B, n, n_fft, hop, win, normalized):
    x = torch.randn(B, n, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    window = torch.hann_window(win)
    X = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=window.double(), normalized=normalized, return_complex=True)
    assert ops.stft_frames(n, n_fft, hop) == X.shape[-1]
    assert _lib.query('alm_stft_bwd_ws_floats', B, n, n_fft, hop) == n_fft * B * X.shape[-1]
    basis = ops.stft_basis(n_fft, window, normalized, 'cpu')     # the operand of the GEMM, built on the host: frames x basis is torch.stft
    assert basis.dtype == torch.float32 and tuple(basis.shape) == (n_fft, 2 * X.shape[1])
    assert ops.stft_basis(n_fft, window.clone(), normalized, 'cpu') is basis                        # cached by the window's values
    frames = F.pad(x[:, None], (n_fft // 2, n_fft // 2), mode='reflect')[:, 0].unfold(1, n_fft, hop)
    Y = (frames @ basis.double()).reshape(B, -1, X.shape[1], 2).permute(0, 2, 1, 3)
    assert float((torch.view_as_real(X) - Y).abs().max()) <= 1e-6 * float(X.abs().max())


def test_stft_frames_refuse_a_clip_the_reflection_cannot_pad():
    assert ops.stft_frames(512, 1024, 256) == -1 and ops.stft_frames(513, 1024, 256) == 3
    assert ops.stft_frames(0, 64, 16) == -1 and ops.stft_frames(100, 64, 0) == -1
    assert _lib.query('alm_stft_bwd_ws_floats', 1, 512, 1024, 256) == -1


@pytest.mark.parametrize('B,Cin,Cout,H,W,kh,kw,sh,sw,ph,pw', CCONV_CASES)
def test_conv_shape_and_workspace_queries(B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw):
    y = F.conv2d(torch.zeros(1, 1, H, W), torch.zeros(1, 1, kh, kw), stride=(sh, sw), padding=(ph, pw))
    assert ops.cconv2d_out_hw(H, W, (kh, kw), (sh, sw), (ph, pw)) == tuple(y.shape[2:])
    n = _lib.query('alm_cconv2d_wgrad_ws_floats', B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw)
    slab = 2 * Cout * 2 * Cin * kh * kw + 2 * Cout
    assert n > 0 and n % slab == 0 and 1 <= n // slab <= 256
    assert n == _lib.query('alm_cconv2d_wgrad_ws_floats', B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw)


def test_queries_outside_the_envelope():
    q = lambda *a: _lib.query('alm_cconv2d_wgrad_ws_floats', *a)
    assert q(2, 256, 1, 15, 2, 16, 1, 1, 1, 0, 0) == -1          # fewer rows than the kernel
    assert q(2, 4, 4, 8, 8, 3, 3, 0, 1, 1, 1) == -1              # stride 0
    assert q(0, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1) == -1
    assert q(2, 4096, 4096, 8, 8, 7, 7, 1, 1, 3, 3) == -1        # the workspace passes 2^31 floats
    assert ops.cconv2d_out_hw(15, 2, (16, 1)) is None and ops.cconv2d_out_hw(16, 2, (16, 1)) == (1, 2)
    assert _lib.query('alm_modrelu_ws_floats') >= 1024


def test_soundstream_builds_the_native_module():
    ss = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True, stft_normalized=True, complex_stft_discr_logits_abs=False,
                       complex_stft_discr_kwargs=dict(channels=8, n_fft=512, hop_length=128, win_length=400))
    d = ss.stft_discriminator
    assert isinstance(d, A.ComplexSTFTDiscriminator)
    assert d.stft_normalized is True and d.logits_abs is False and (d.n_fft, d.hop_length, d.win_length) == (512, 128, 400)
    assert tuple(d.init_conv.weight.shape) == (8, 1, 7, 7, 2)
    default = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True).stft_discriminator
    assert default.stft_normalized is False and default.logits_abs is True and default.n_fft == 1024
    assert any(k.startswith('stft_discriminator.layers.5.1.') for k in ss.state_dict())
    rest = {id(p) for p in ss.non_discr_parameters()}
    assert not rest & {id(p) for p in d.parameters()}
    handed = A.SoundStream(**SMALL_SS, stft_discriminator=A.ComplexSTFTDiscriminator(**SMALL), with_discriminators=True)
    assert isinstance(handed.stft_discriminator, A.ComplexSTFTDiscriminator) and handed.stft_discriminator.n_fft == 64


def test_without_the_switch_nothing_is_registered():
    ss = A.SoundStream(**SMALL_SS, stft_discriminator=True, stft_normalized=True, complex_stft_discr_kwargs=dict(channels=8))
    assert not hasattr(ss, 'stft_discriminator') and [n for n, _ in ss.named_children()] == ['encoder', 'decoder', 'rq']
    none = A.SoundStream(**SMALL_SS, with_discriminators=True)   # None keeps its behaviour: nothing registered, the loss branches name the way out
    assert not hasattr(none, 'stft_discriminator')
    with pytest.raises(NotImplementedError, match='stft_discriminator=True'):
        none(torch.zeros(1, 640), return_discr_loss=True)


def test_refusals_fire_before_any_launch():
    d = A.ComplexSTFTDiscriminator(**SMALL)
    with pytest.raises(RuntimeError, match='MI355X only'):
        d(torch.zeros(1, 1, 320))
    with pytest.raises(ValueError, match='too short'):
        d(torch.zeros(1, 1, 32))
    assert d.check_geometry(320) == (2, 6) and d.check_geometry(33) == (2, 2)
    with pytest.raises(NotImplementedError, match='input_channels'):
        A.ComplexSTFTDiscriminator(**SMALL, input_channels=2)(torch.zeros(1, 2, 320))
    shallow = A.ComplexSTFTDiscriminator(**{**SMALL, 'n_fft': 32, 'win_length': 32})        # 17 rows shrink to 9: fewer than the final conv's 16
    with pytest.raises(ValueError, match='final conv'):
        shallow(torch.zeros(1, 1, 320))
    ss = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ss(torch.zeros(1, 2560), return_discr_loss=True)
    with pytest.raises(NotImplementedError, match='apply_grad_penalty'):
        ss(torch.zeros(1, 2560), return_discr_loss=True, apply_grad_penalty=True)
    from audiolm_pytorch_amd import discriminators as D
    with pytest.raises(RuntimeError, match='MI355X only'):
        D.l1_loss(torch.zeros(3, dtype=torch.complex64), torch.zeros(3, dtype=torch.complex64))
    with pytest.raises(TypeError, match='complex64'):
        D.l1_loss(torch.zeros(3, dtype=torch.complex128), torch.zeros(3, dtype=torch.complex128))
