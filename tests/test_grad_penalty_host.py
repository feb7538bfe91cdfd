"""CPU: the gradient-penalty switch of SoundStream (`with_grad_penalty=True`), its refusals, the state it must not change, and the host-side argument
checks of the new entry points (csrc/discr.hip alm_gconv1d_fwd_masked / alm_grad_penalty_*, csrc/stft_discr.hip alm_modrelu_bwd2 / alm_cabs_bwd2).
No launch happens here: every call below is refused before one."""
import ctypes
import os
import re

import pytest
import torch

import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib
from audiolm_pytorch_amd import discriminators as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SS = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False, multi_spectral_recon_loss_weight=0.)
SYMBOLS = ('alm_gconv1d_fwd_masked', 'alm_grad_penalty_ws_floats', 'alm_grad_penalty_fwd', 'alm_grad_penalty_bwd', 'alm_modrelu_bwd2', 'alm_cabs_bwd2')


def test_without_the_switch_the_refusal_remains_and_names_the_switch():
    ss = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True)
    assert ss.with_grad_penalty is False
    for kw in (dict(return_discr_loss=True), dict(return_discr_loss=True, return_discr_losses_separately=True), {}):
        with pytest.raises(NotImplementedError, match='apply_grad_penalty') as e:
            ss(torch.zeros(1, 2560), apply_grad_penalty=True, **kw)
        assert 'with_grad_penalty=True' in str(e.value)


def test_with_the_switch_the_call_reaches_the_device_refusal():
    ss = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True, with_grad_penalty=True)
    assert ss.with_grad_penalty is True
    for kw in (dict(return_discr_loss=True), dict(return_discr_loss=True, return_discr_losses_separately=True)):
        with pytest.raises(RuntimeError, match='MI355X only'):
            ss(torch.zeros(1, 2560), apply_grad_penalty=True, **kw)
    with pytest.raises(RuntimeError, match='MI355X only'):      # the generator branch accepts the flag and ignores it, like the reference
        ss(torch.zeros(1, 2560), apply_grad_penalty=True)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ss(torch.zeros(1, 2560), apply_grad_penalty=True, return_loss_breakdown=True)
    # the other refusals keep their order: a model without an STFT discriminator still names that first
    none = A.SoundStream(**SMALL_SS, with_discriminators=True, with_grad_penalty=True)
    with pytest.raises(NotImplementedError, match='stft_discriminator=True'):
        none(torch.zeros(1, 2560), return_discr_loss=True, apply_grad_penalty=True)


def test_the_switch_needs_the_discriminators():
    with pytest.raises(ValueError, match='with_discriminators=True'):
        A.SoundStream(**SMALL_SS, with_grad_penalty=True)


def test_the_switch_registers_nothing():
    torch.manual_seed(0)
    plain = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True)
    torch.manual_seed(0)
    switched = A.SoundStream(**SMALL_SS, stft_discriminator=True, with_discriminators=True, with_grad_penalty=True)
    assert list(plain.state_dict()) == list(switched.state_dict())
    assert [n for n, _ in plain.named_children()] == [n for n, _ in switched.named_children()]
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in switched.named_buffers()]
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in switched.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), switched.state_dict().values()))


def test_gradient_penalty_is_public_and_refuses_the_cpu():
    assert A.gradient_penalty is D.gradient_penalty
    wave = torch.zeros(2, 1, 16, requires_grad=True)
    with pytest.raises(RuntimeError, match='MI355X only'):      # torch's autograd takes the gradient; the reduction is the HIP kernel
        A.gradient_penalty(wave, (wave * wave).sum())
    assert D._WAVE_GRAD_ONLY == [False]


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} is not declared in include/audiolm_hip.h'
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(',')), name
        assert hasattr(lib, name), name


def test_the_launchers_refuse_on_the_host():
    """every new entry point checks its arguments before the launch: the error code comes back on a machine without a GPU.  X is a non-null address
    that is never dereferenced (each call below has exactly one defect and is refused for it)."""
    q, BAD, UNSUPPORTED, X = _lib.query, 10001, 10002, ctypes.c_void_p(4096)

    def each(name, good, defects, code=BAD):
        for i, v in defects:
            args = list(good)
            args[i] = v
            assert q(name, *args) == code, (name, i, v)

    # v, w, y (may be null), out, B, Cin, Cout, Tin, ksize, stride, padding, groups, stream
    good = [X, X, X, X, 2, 16, 64, 100000, 41, 4, 20, 4, None]
    each('alm_gconv1d_fwd_masked', good, [(0, None), (1, None), (3, None), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, -1), (11, 0), (11, 3),
                                          (4, -2), (8, 200000)])                               # groups not dividing; a kernel longer than the padded input
    each('alm_gconv1d_fwd_masked', good, [(8, 7000), (4, 70000)], UNSUPPORTED)       # a window beyond the LDS tile (Tin = 100000 admits it); a batch beyond the grid
    # R, n
    assert q('alm_grad_penalty_ws_floats', 3, 70001) == 3 * 18 and q('alm_grad_penalty_ws_floats', 1, 1) == 1
    assert q('alm_grad_penalty_ws_floats', 2, 4096 * 1024 + 1) == 2 * 513                     # the span doubles past 1024 blocks per row
    for R, n in ((0, 5), (-1, 5), (3, 0), (65536, 5)):
        assert q('alm_grad_penalty_ws_floats', R, n) == -1
    # G, out, norms, ws, ws_floats, R, n, weight, center, stream
    each('alm_grad_penalty_fwd', [X, X, X, X, 54, 3, 70001, 10., 0., None],
         [(0, None), (1, None), (2, None), (3, None), (5, 0), (5, -3), (6, 0), (6, -1), (4, 53)])
    each('alm_grad_penalty_fwd', [X, X, X, X, 1 << 20, 3, 5, 10., 0., None], [(5, 65536)], UNSUPPORTED)
    # G, norms, gout, dG, R, n, weight, center, stream
    each('alm_grad_penalty_bwd', [X, X, X, X, 3, 70001, 10., 0., None], [(0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (4, -1), (5, -1)])
    each('alm_grad_penalty_bwd', [X, X, X, X, 3, 5, 10., 0., None], [(4, 65536), (5, 1 << 40)], UNSUPPORTED)
    # g, z, b, v (may be null), beta, dg, dz (may be null), db, ws, n, stream
    each('alm_modrelu_bwd2', [X, X, X, None, X, X, None, X, X, 210, None], [(0, None), (1, None), (2, None), (4, None), (5, None), (7, None), (8, None),
                                                                           (9, 0), (9, -5)])
    # g, z, v, dg, dz (may be null), n, stream
    each('alm_cabs_bwd2', [X, X, X, X, None, 210, None], [(0, None), (1, None), (2, None), (3, None), (5, 0), (5, -5)])
    each('alm_cabs_bwd2', [X, X, X, X, None, 210, None], [(5, 1 << 40)], UNSUPPORTED)
