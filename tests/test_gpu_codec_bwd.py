"""Backward of SoundStream's conv stacks on the MI355X (csrc/codec_bwd.hip + the autograd layer of audiolm_pytorch_amd/codec_bwd.py).

Op level: dx / dW / db of conv (+ ELU) against float64 CPU autograd of the oracle's causal_conv1d / causal_conv_transpose1d with a random g.
End to end: loss and every encoder / decoder gradient against the REAL reference (tests/golden/codec_bwd_small.pt), the decoder alone against
float64 autograd of the oracle, two SGD steps against the oracle (weight-image invalidation).

Tolerance: rel-max <= 2e-5, the project's fp32 conv tolerance.  CPU fp32 autograd deviates from float64 by <= 7.2e-7 at these shapes (1.5e-6 for dW at
T = 4096), so the bound leaves >= 10x for a different summation order.  Every gradient is bitwise reproducible (no atomics): two runs are torch.equal."""
import os

import pytest
import torch
import torch.nn.functional as F

import audiolm_oracle as O
from common import GOLDEN_DIR, synth_state_dict

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def check(name, got, ref):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    e = relmax(got, ref)
    print(f'{name}: rel-max {e:.3e}')
    assert e <= TOL, (name, e)


@pytest.fixture(scope='module')
def ops():
    from audiolm_pytorch_amd import ops as _ops
    return _ops


def _conv_ref(x, w, b, g, *, k, stride, dil, elu, zero_pad):
    """float64 CPU autograd: (y fp32, dx, dW, db)"""
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    if zero_pad:
        out = F.conv1d(F.pad(x64, (dil * (k - 1) + 1 - stride, 0)), w64, b64, stride=stride, dilation=dil)
    else:
        out = O.causal_conv1d(x64, w64, b64, dilation=dil, stride=stride)
    y = F.elu(out) if elu else out
    y.backward(g.double())
    return x64.grad, w64.grad, b64.grad


def _conv_gpu(ops, x, w, b, g, *, k, stride, dil, elu, zero_pad, need_x=True):
    xd, wd, bd, gd = (t.to(dev()) for t in (x, w, b, g))
    Cout, Cin, _ = w.shape
    y = ops.conv1d_causal(xd, ops.conv1d_pack(wd), bd, Cout, k, stride=stride, dilation=dil, elu=elu, zero_pad=zero_pad)
    ys = y if elu else None
    dx = ops.conv1d_dgrad(gd, ys, ops.conv1d_pack_t(wd), Cin, x.shape[2], k, stride=stride, dilation=dil, zero_pad=zero_pad) if need_x else None
    dw, db = ops.conv1d_wgrad(gd, ys, xd, k, stride=stride, dilation=dil, zero_pad=zero_pad)
    return dx, dw, db


CONV_SHAPES = [(2, 1, 32, 300, 7, 1, 1), (1, 32, 1, 300, 7, 1, 1), (1, 32, 32, 277, 7, 1, 9), (1, 32, 32, 55, 7, 1, 9), (2, 32, 64, 320, 4, 2, 1),
               (1, 64, 128, 256, 8, 4, 1), (1, 128, 256, 200, 10, 5, 1), (1, 256, 512, 64, 16, 8, 1), (2, 48, 40, 131, 3, 1, 1),
               (2, 32, 32, 4099, 7, 1, 3)]


@pytest.mark.parametrize('B,Cin,Cout,T,k,stride,dil', CONV_SHAPES)
def test_conv_elu_backward(ops, B, Cin, Cout, T, k, stride, dil):
    x, w, b = rnd(B, Cin, T, seed=1), rnd(Cout, Cin, k, seed=2, scale=(Cin * k) ** -0.5), rnd(Cout, seed=3, scale=0.1)
    g = rnd(B, Cout, T // stride, seed=4)
    kw = dict(k=k, stride=stride, dil=dil, elu=True, zero_pad=False)
    rdx, rdw, rdb = _conv_ref(x, w, b, g, **kw)
    dx, dw, db = _conv_gpu(ops, x, w, b, g, **kw)
    check('dx', dx, rdx), check('dW', dw, rdw), check('db', db, rdb)
    dx2, dw2, db2 = _conv_gpu(ops, x, w, b, g, **kw)                     # determinism: no atomics, a fixed summation order
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('elu', [False, True])
def test_zero_pad_conv_backward(ops, elu):
    B, Cin, Cout, T, k, dil = 2, 40, 48, 150, 3, 2
    x, w, b = rnd(B, Cin, T, seed=5), rnd(Cout, Cin, k, seed=6, scale=(Cin * k) ** -0.5), rnd(Cout, seed=7, scale=0.1)
    g = rnd(B, Cout, T, seed=8)
    kw = dict(k=k, stride=1, dil=dil, elu=elu, zero_pad=True)
    rdx, rdw, rdb = _conv_ref(x, w, b, g, **kw)
    dx, dw, db = _conv_gpu(ops, x, w, b, g, **kw)
    check('dx', dx, rdx), check('dW', dw, rdw), check('db', db, rdb)


def test_phase_deinterleave_is_the_adjoint(ops):
    B, Cout, s, n = 2, 5, 5, 37
    y, g = rnd(B, s * Cout, n, seed=9).to(dev()), rnd(B, Cout, n * s, seed=10).to(dev())
    gd = ops.phase_deinterleave(g, Cout, s)
    assert torch.equal(ops.phase_interleave(gd, Cout, s), g)            # a permutation: its adjoint is its inverse
    assert gd.shape == y.shape


def _mods():
    from audiolm_pytorch_amd import soundstream as S
    return S


@pytest.mark.parametrize('s', [2, 4, 5, 8])
def test_conv_transpose_backward(s):
    S = _mods()
    B, Cin, Cout, n = 2, 64, 32, 37
    x, w, b = rnd(B, Cin, n, seed=11), rnd(Cin, Cout, 2 * s, seed=12, scale=(2 * Cin) ** -0.5), rnd(Cout, seed=13, scale=0.1)
    g = rnd(B, Cout, n * s, seed=14)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    O.causal_conv_transpose1d(x64, w64, b64, s).backward(g.double())
    m = S.CausalConvTranspose1d(Cin, Cout, 2 * s, s).to(dev()).train()
    with torch.no_grad():
        m.conv.weight.copy_(w), m.conv.bias.copy_(b)
    outs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        xd = x.to(dev()).requires_grad_()
        y = m(xd)
        assert y.grad_fn is not None
        y.backward(g.to(dev()))
        outs.append((xd.grad, m.conv.weight.grad, m.conv.bias.grad))
    check('dx', outs[0][0], x64.grad), check('dW', outs[0][1], w64.grad), check('db', outs[0][2], b64.grad)
    assert all(torch.equal(a, c) for a, c in zip(*outs))


def _unit(C, dil, seed):
    S = _mods()
    u = S.ResidualUnit(C, C, dil).to(dev())
    sd = {'fn.0.conv.weight': rnd(C, C, 7, seed=seed, scale=(7 * C) ** -0.5), 'fn.0.conv.bias': rnd(C, seed=seed + 1, scale=0.1),
          'fn.2.conv.weight': rnd(C, C, 1, seed=seed + 2, scale=C ** -0.5), 'fn.2.conv.bias': rnd(C, seed=seed + 3, scale=0.1)}
    u.load_state_dict(sd)
    return u, sd


@pytest.mark.parametrize('B,C,T,dil', [(2, 32, 277, 9), (1, 96, 200, 1), (1, 256, 130, 3)])
def test_residual_unit_backward(B, C, T, dil):
    u, sd = _unit(C, dil, 20)
    x, g = rnd(B, C, T, seed=30), rnd(B, C, T, seed=31)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    O.residual_unit(sd64, '', x64, dil).backward(g.double())
    with torch.no_grad():
        y_eval = u.eval()(x.to(dev()))
    assert y_eval.grad_fn is None
    outs = []
    for _ in range(2):
        u.train().zero_grad(set_to_none=True)
        xd = x.to(dev()).requires_grad_()
        y = u(xd)
        assert y.grad_fn is not None and torch.equal(y.detach(), y_eval)          # same fma chains as the (fused) eval path
        y.backward(g.to(dev()))
        outs.append((xd.grad,) + tuple(p.grad for p in u.parameters()))
    check('dx', outs[0][0], x64.grad)
    for (k, p), got in zip(u.named_parameters(), outs[0][1:]):
        check(k, got, sd64[k].grad)
    assert all(torch.equal(a, c) for a, c in zip(*outs))


def test_input_gradient_is_skipped_when_not_needed(ops, monkeypatch):
    """needs_input_grad[0] = False (the wave does not require grad): no alm_conv1d_dgrad launch for that conv, the weight gradients unchanged"""
    S = _mods()
    from audiolm_pytorch_amd import _lib
    B, Cin, Cout, T = 2, 1, 32, 300
    x, w, b, g = rnd(B, Cin, T, seed=1), rnd(Cout, Cin, 7, seed=2, scale=7 ** -0.5), rnd(Cout, seed=3, scale=0.1), rnd(B, Cout, T, seed=4)
    _, rdw, rdb = _conv_ref(x, w, b, g, k=7, stride=1, dil=1, elu=False, zero_pad=False)
    m = S.CausalConv1d(Cin, Cout, 7).to(dev()).train()
    with torch.no_grad():
        m.conv.weight.copy_(w), m.conv.bias.copy_(b)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    xd = x.to(dev())
    m(xd).backward(g.to(dev()))
    assert 'alm_conv1d_wgrad' in calls and 'alm_conv1d_dgrad' not in calls, calls
    assert xd.grad is None
    check('dW', m.conv.weight.grad, rdw), check('db', m.conv.bias.grad, rdb)
    dx, _, _ = _conv_gpu(ops, x, w, b, g, k=7, stride=1, dil=1, elu=False, zero_pad=False, need_x=False)
    assert dx is None


# ---------------------------------------------------------------------------------------------- end to end

@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'codec_bwd_small.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def _codec(golden):
    S = _mods()
    fx, sd = golden
    ss = S.SoundStream(**fx['ctor'])
    missing, unexpected = ss.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(('encoder.', 'decoder.'))]
    return ss.to(dev())


def _wave(fx):
    wave = fx['inputs']['wave']
    return wave[:, None, :wave.shape[-1] // 320 * 320].contiguous()


def test_encoder_decoder_gradients_match_the_reference(golden):
    fx, _ = golden
    ss = _codec(golden)
    x = _wave(fx).to(dev())
    with torch.no_grad():
        y_eval = ss.decode(ss.encode(x))                                 # eval mode (the constructor ends in eval())
    assert y_eval.grad_fn is None
    enc_eval = ss.encode(x)                                              # eval mode with grad mode on: still no graph
    assert enc_eval.grad_fn is None and ss.decode(enc_eval).grad_fn is None
    ss.train()
    with torch.no_grad():
        assert ss.decode(ss.encode(x)).grad_fn is None
    runs = []
    for _ in range(2):
        ss.zero_grad(set_to_none=True)
        enc = ss.encode(x)
        y = ss.decode(enc)
        assert y.grad_fn is not None
        loss = F.mse_loss(y, x)
        loss.backward()
        runs.append({k: p.grad.clone() for k, p in ss.named_parameters() if k.startswith(('encoder.', 'decoder.'))})
    assert torch.equal(enc.detach(), enc_eval), 'training-mode encoder output differs from the eval-mode output'
    assert torch.equal(y.detach(), y_eval), 'training-mode output differs from the eval-mode output'
    ref = fx['outputs']
    e = abs(float(loss.detach()) - float(ref['loss'])) / abs(float(ref['loss']))
    print(f'loss rel {e:.3e}')
    assert e <= 1e-5
    assert set(runs[0]) == set(ref['grads'])
    worst = max((relmax(runs[0][k], gr), k) for k, gr in ref['grads'].items())
    print('worst gradient rel-max', worst)
    for k, gr in ref['grads'].items():
        assert relmax(runs[0][k], gr) <= TOL, (k, relmax(runs[0][k], gr))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_decoder_alone_from_indices(golden):
    fx, sd = golden
    ss = _codec(golden).train()
    g = torch.Generator().manual_seed(12)
    indices = torch.randint(0, 32, (2, 9, 4), generator=g)
    indices[1, -2:, 2:] = -1
    sd64 = {k: (v.double().requires_grad_(k.startswith('decoder.')) if v.is_floating_point() else v) for k, v in sd.items()}
    ref = O.soundstream_decode_from_indices(sd64, indices, strides=fx['ctor']['strides'], num_quantizers=4)
    gy = rnd(*ref.shape, seed=40)
    ref.backward(gy.double())
    y = ss.decode_from_codebook_indices(indices.to(dev()))
    assert y.grad_fn is not None
    check('wave', y.detach(), ref.detach())
    y.backward(gy.to(dev()))
    for k, p in ss.named_parameters():
        if k.startswith('decoder.'):
            check(k, p.grad, sd64[k].grad)
        else:
            assert p.grad is None, k


def test_two_sgd_steps_pick_up_in_place_updates(golden):
    """an in-place optimiser step must invalidate the forward AND the transposed weight images: the second step's loss follows the oracle's"""
    fx, sd = golden
    ss = _codec(golden).train()
    x = _wave(fx)
    strides = tuple(fx['ctor']['strides'])
    names = [k for k in sd if k.startswith(('encoder.', 'decoder.'))]
    lr = 1e-4
    ref = {k: v.double().clone() for k, v in sd.items() if k in names}
    ref_losses, losses = [], []
    xd = x.to(dev())
    params = dict(ss.named_parameters())
    for step in range(3):
        p64 = {k: v.clone().requires_grad_() for k, v in ref.items()}
        l64 = F.mse_loss(O.soundstream_decoder(p64, O.soundstream_encoder(p64, x.double(), strides=strides), strides=strides), x.double())
        l64.backward()
        ref_losses.append(float(l64.detach()))
        ref = {k: (v - lr * p64[k].grad).detach() for k, v in ref.items()}
        ss.zero_grad(set_to_none=True)
        loss = F.mse_loss(ss.decode(ss.encode(xd)), xd)
        losses.append(float(loss.detach()))
        if step < 2:
            loss.backward()
            with torch.no_grad():
                for k in names:
                    params[k].add_(params[k].grad, alpha=-lr)
    print('losses', losses, 'oracle', ref_losses)
    assert abs(ref_losses[1] - ref_losses[0]) > 1e-4 * ref_losses[0]      # the step moves the loss by far more than the bound below
    for got, want in zip(losses, ref_losses):
        assert abs(got - want) <= 1e-5 * abs(want), (losses, ref_losses)


def test_local_attention_in_training_mode_raises():
    S = _mods()
    ss = S.SoundStream(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, attn_window_size=8, attn_dim_head=8, attn_heads=2).to(dev())
    x = rnd(1, 1, 640, seed=50).to(dev())
    ss.train()
    with pytest.raises(NotImplementedError, match='LocalTransformer backward'):
        ss.encode(x)
    with pytest.raises(NotImplementedError, match='LocalTransformer backward'):
        ss.decode(torch.zeros(1, 2, 16, device=dev()))
    with pytest.raises(NotImplementedError):                             # the loss branches of forward stay out of scope
        ss(x.squeeze(1))
