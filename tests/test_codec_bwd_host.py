"""CPU: the host side of the codec backward (csrc/codec_bwd.hip): exported entry points, the weight-gradient workspace arithmetic, the wrappers'
refusal of CPU tensors, and the fixture tests/golden/codec_bwd_small.pt (REAL reference encoder / decoder gradients) against the oracle."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import audiolm_oracle as O
from common import GOLDEN_DIR, synth_state_dict

import audiolm_pytorch_amd  # noqa: F401
from audiolm_pytorch_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('alm_conv1d_dgrad', 'alm_conv1d_wgrad', 'alm_conv1d_wgrad_ws_floats', 'alm_conv1d_wgrad_chunk', 'alm_phase_deinterleave')

# (B, Cin, Cout, T, k, stride, dil): the op-level shapes of tests/test_gpu_codec_bwd.py
OP_SHAPES = [(2, 1, 32, 300, 7, 1, 1), (1, 32, 1, 300, 7, 1, 1), (1, 32, 32, 277, 7, 1, 9), (1, 32, 32, 55, 7, 1, 9), (2, 32, 64, 320, 4, 2, 1),
             (1, 64, 128, 256, 8, 4, 1), (1, 128, 256, 200, 10, 5, 1), (1, 256, 512, 64, 16, 8, 1), (2, 48, 40, 131, 3, 1, 1),
             (2, 32, 32, 4099, 7, 1, 3)]


def test_header_declares_and_library_exports_the_backward_entry_points():
    src = open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\bint\s+(alm_\w+)\s*\(', src))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_wgrad_workspace_covers_every_partial():
    """alm_conv1d_wgrad writes, per time chunk (alm_conv1d_wgrad_chunk steps, chunks never cross a batch element), one fp32 tile per tap over the
    channel counts padded to the 32 x 32 MFMA tile, plus one padded row of bias partials: the caller's workspace (alm_conv1d_wgrad_ws_floats) must cover
    chunks x (k x CoutP x CinP + CoutP) for every shape (host arithmetic only: no GPU)."""
    up32 = lambda n: -(-n // 32) * 32                            # noqa: E731
    multi = 0
    for B, Cin, Cout, T, k, s, d in OP_SHAPES + [(8, 1, 32, 720000, 7, 1, 1), (8, 256, 512, 18000, 16, 8, 1)]:
        Tout = T // s
        ch = _lib.query('alm_conv1d_wgrad_chunk', B, Tout)
        assert ch > 0 and ch % 32 == 0
        chunks = B * -(-Tout // ch)
        need = chunks * (k * up32(Cout) * up32(Cin) + up32(Cout))
        got = _lib.query('alm_conv1d_wgrad_ws_floats', B, Cin, Cout, Tout, k)
        assert got >= need, (B, Cin, Cout, T, k, s, d, got, need)
        multi += -(-Tout // ch) > 1
    assert multi >= 2                                            # the 4099-step case and the 30 s stage are cut into several chunks
    assert _lib.query('alm_conv1d_wgrad_ws_floats', 2, 32, 32, 4099, 7) > _lib.query('alm_conv1d_wgrad_ws_floats', 2, 32, 32, 2048, 7)


def test_backward_wrappers_refuse_cpu_tensors():
    g, x, w = torch.zeros(1, 32, 64), torch.zeros(1, 32, 64), torch.zeros(32, 32, 3)
    with pytest.raises(_lib.AlmError):
        ops.conv1d_pack_t(w)
    with pytest.raises(_lib.AlmError):
        ops.conv1d_dgrad(g, None, w, 32, 64, 3)
    with pytest.raises(_lib.AlmError):
        ops.conv1d_wgrad(g, None, x, 3)
    with pytest.raises(_lib.AlmError):
        ops.phase_deinterleave(torch.zeros(1, 4, 64), 4, 2)


def test_oracle_fp32_autograd_reproduces_the_reference_gradients():
    """the fixture (REAL reference, CPU fp32) and the oracle's encoder / decoder agree: loss to 1e-5, every gradient to rel-max 2e-5"""
    fx = torch.load(os.path.join(GOLDEN_DIR, 'codec_bwd_small.pt'), weights_only=False)
    sd = {k: v.clone().requires_grad_(k.startswith(('encoder.', 'decoder.'))) for k, v in synth_state_dict(fx['shapes'], fx['seed']).items()}
    strides = tuple(fx['ctor']['strides'])
    wave = fx['inputs']['wave']
    n = wave.shape[-1] // 320 * 320
    x = wave[:, None, :n]
    y = O.soundstream_decoder(sd, O.soundstream_encoder(sd, x, strides=strides), strides=strides)
    loss = F.mse_loss(y, x)
    loss.backward()
    ref = fx['outputs']
    assert abs(float(loss.detach()) - float(ref['loss'])) <= 1e-5 * abs(float(ref['loss']))
    assert len(ref['grads']) == 120
    for k, gr in ref['grads'].items():
        got = sd[k].grad
        assert got is not None and got.shape == gr.shape, k
        assert float((got - gr).abs().max()) <= 2e-5 * float(gr.abs().max()), k
