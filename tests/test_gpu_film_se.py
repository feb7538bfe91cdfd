"""The denoising SoundStream on the MI355X: squeeze-excite inside the ResidualUnit and the FiLM conditioners (csrc/film_se.hip, the autograd layer
of audiolm_pytorch_amd/codec_bwd.py, soundstream.SoundStream(squeeze_excite=True, with_film=True)).

Op level: output and every gradient of alm_se_gate_* / alm_film_* against float64 CPU autograd of tests/film_se_restated.py with a random g.
End to end: loss, reconstruction and every gradient against the REAL reference (tests/golden/film_se_small.pt) for both conditions; training-mode
output bitwise the eval-mode output; two SGD steps against the restatement (a stale weight image would show); is_denoising=None issues no FiLM launch.

Tolerance: rel-max <= 2e-5, the project's fp32 conv tolerance (tests/test_gpu_codec_bwd.py).  Measured on the CPU, fp32 eager autograd of the
restatement against float64: at the op-level shapes below at most 2.1e-6 (SE, on db1 at (2, 32, 8, 4099); 1.5e-6 on db2 there, <= 5.8e-7 elsewhere) and
1.2e-7 (FiLM); the committed fixture (the reference's own fp32) against float64 of the restatement: 2.6e-6 over all gradients (an SE bias gradient),
5.5e-7 on the reconstruction, 1.1e-7 on the loss -- all below one fifth of the bound.
Every gradient is bitwise reproducible (no atomics): two runs are torch.equal."""
import os

import pytest
import torch
import torch.nn.functional as F

import film_se_restated as R
from common import GOLDEN_DIR, synth_state_dict

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
SE_SHAPES = [(2, 4, 8, 333), (1, 32, 8, 1), (2, 48, 12, 1000), (1, 256, 64, 130), (1, 512, 128, 70), (2, 32, 8, 4099)]
FILM_SHAPES = [(14, 16), (1, 512), (3000, 96)]


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


# ---------------------------------------------------------------------------------------------- op level

def se_inputs(B, C, inner, T):
    """(u, w1, b1, w2, b2, g, residual): unit-variance activations, fan-in-scaled weights (the pre-activations stay O(1): no saturated gate)"""
    return (rnd(B, C, T, seed=1), rnd(inner, C, 1, seed=2, scale=C ** -0.5), rnd(inner, seed=3, scale=0.1), rnd(C, inner, 1, seed=4, scale=inner ** -0.5),
            rnd(C, seed=5, scale=0.1), rnd(B, C, T, seed=6), rnd(B, C, T, seed=7))


def se_reference(u, w1, b1, w2, b2, g, residual, dtype=F64):
    """(out, du, dW1, db1, dW2, db2) by CPU autograd of the restatement in `dtype`"""
    leaves = [t.to(dtype).requires_grad_() for t in (u, w1, b1, w2, b2)]
    out = R.squeeze_excite(*leaves)
    if residual is not None:
        out = out + residual.to(dtype)
    out.backward(g.to(dtype))
    return (out.detach(),) + tuple(t.grad for t in leaves)


def film_inputs(rows, C):
    return rnd(rows, C, seed=11), rnd(2 * C, 2, seed=12, scale=2 ** -0.5), rnd(2 * C, seed=13, scale=0.1), rnd(rows, C, seed=14)


def film_reference(x, w, b, g, is_denoising, dtype=F64):
    leaves = [t.to(dtype).requires_grad_() for t in (x, w, b)]
    y = R.film(*leaves, R.cond_of(is_denoising, dtype))
    y.backward(g.to(dtype))
    return (y.detach(),) + tuple(t.grad for t in leaves)


@pytest.mark.parametrize('with_residual', [False, True])
@pytest.mark.parametrize('B,C,inner,T', SE_SHAPES)
def test_se_gate_forward_backward(ops, B, C, inner, T, with_residual):
    u, w1, b1, w2, b2, g, res = se_inputs(B, C, inner, T)
    res = res if with_residual else None
    ref = se_reference(u, w1, b1, w2, b2, g, res)
    ud, w1d, b1d, w2d, b2d, gd = (t.to(dev()) for t in (u, w1, b1, w2, b2, g))
    resd = res.to(dev()) if with_residual else None
    runs = []
    for _ in range(2):
        out = ops.se_gate_fwd(ud, w1d, b1d, w2d, b2d, residual=resd)
        runs.append((out,) + ops.se_gate_bwd(gd, ud, w1d, b1d, w2d, b2d))
    for name, got, want in zip(('out', 'du', 'dW1', 'db1', 'dW2', 'db2'), runs[0], ref):
        check(name, got, want)
    assert all(torch.equal(a, c) for a, c in zip(*runs))         # determinism: no atomics, a fixed summation order


@pytest.mark.parametrize('is_denoising', [True, False])
@pytest.mark.parametrize('rows,C', FILM_SHAPES)
def test_film_forward_backward(ops, rows, C, is_denoising):
    x, w, b, g = film_inputs(rows, C)
    ref = film_reference(x, w, b, g, is_denoising)
    xd, wd, bd, gd = (t.to(dev()) for t in (x, w, b, g))
    c0, c1 = float(is_denoising), float(not is_denoising)
    runs = []
    for _ in range(2):
        runs.append((ops.film_fwd(xd, wd, bd, c0, c1),) + ops.film_bwd(gd, xd, wd, bd, c0, c1))
    for name, got, want in zip(('y', 'dx', 'dW', 'db'), runs[0], ref):
        check(name, got, want)
    assert float(runs[0][2][:, 1 if is_denoising else 0].abs().max()) == 0          # the condition's zero entry: that column gets no gradient
    assert all(torch.equal(a, c) for a, c in zip(*runs))


def test_se_unit_train_output_is_the_eval_output():
    from audiolm_pytorch_amd import soundstream as S
    C, dil = 48, 3
    unit = S.ResidualUnit(C, C, dil, squeeze_excite=True).to(dev())
    sd = {k: rnd(*v.shape, seed=20 + i, scale=0.1 if k.endswith('bias') else v[0].numel() ** -0.5) for i, (k, v) in enumerate(unit.state_dict().items())}
    unit.load_state_dict(sd)
    x, g = rnd(2, C, 277, seed=40), rnd(2, C, 277, seed=41)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    R.se_residual_unit(sd64, '', x64, dil).backward(g.double())
    with torch.no_grad():
        y_eval = unit.eval()(x.to(dev()))
    assert y_eval.grad_fn is None
    outs = []
    for _ in range(2):
        unit.train().zero_grad(set_to_none=True)
        xd = x.to(dev()).requires_grad_()
        y = unit(xd)
        assert y.grad_fn is not None and torch.equal(y.detach(), y_eval)
        y.backward(g.to(dev()))
        outs.append((xd.grad,) + tuple(p.grad for p in unit.parameters()))
    check('dx', outs[0][0], x64.grad)
    for (k, _), got in zip(unit.named_parameters(), outs[0][1:]):
        check(k, got, sd64[k].grad)
    assert all(torch.equal(a, c) for a, c in zip(*outs))


# ---------------------------------------------------------------------------------------------- end to end

@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'film_se_small.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def _codec(golden, **kw):
    import audiolm_pytorch_amd as A
    fx, sd = golden
    ss = A.SoundStream(**fx['ctor'], **kw)
    full = dict(ss.state_dict())
    full.update({k: v for k, v in sd.items() if k in full})
    ss.load_state_dict(full, strict=True)
    g = torch.Generator().manual_seed(5)
    for layer in ss.rq.rvqs[0].layers:                           # a trained quantiser's state: the eval-mode forward refuses uninitialised codebooks
        layer._codebook.embed.copy_(torch.randn(layer._codebook.embed.shape, generator=g) * 0.5)
        layer._codebook.initted.fill_(True)
    return ss.to(dev())


def _wave(fx):
    wave = fx['inputs']['wave']
    return wave[:, None, :wave.shape[-1] // 320 * 320].contiguous()


def _autoencode(ss, x, is_denoising):
    cond = (float(is_denoising), float(not is_denoising))
    return ss.decode(ss.decoder_film(ss.encoder_film(ss.encode(x), cond), cond))


PREFIXES = ('encoder.', 'decoder.', 'encoder_film.', 'decoder_film.')


@pytest.mark.parametrize('name,is_denoising', [('denoise', True), ('plain', False)])
def test_gradients_match_the_reference(golden, name, is_denoising):
    fx, _ = golden
    ss = _codec(golden, with_film=True)
    x = _wave(fx).to(dev())
    with torch.no_grad():
        y_eval = _autoencode(ss, x, is_denoising)                # eval mode (the constructor ends in eval())
    assert y_eval.grad_fn is None
    ss.train()
    runs = []
    for _ in range(2):
        ss.zero_grad(set_to_none=True)
        y = _autoencode(ss, x, is_denoising)
        assert y.grad_fn is not None
        loss = F.mse_loss(y, x)
        loss.backward()
        runs.append({k: p.grad.clone() for k, p in ss.named_parameters() if k.startswith(PREFIXES)})
    assert torch.equal(y.detach(), y_eval), 'training-mode output differs from the eval-mode output'
    ref = fx['outputs'][name]
    e = abs(float(loss.detach()) - float(ref['loss'])) / abs(float(ref['loss']))
    print(f'loss rel {e:.3e}')
    assert e <= 1e-5
    check('recon', y.detach(), ref['recon'])
    grads = R.golden_grads(ref)
    assert set(runs[0]) == set(grads)
    errs = {k: relmax(runs[0][k].reshape(-1)[::stride], want) for k, (shape, stride, want) in grads.items()}
    print('worst gradient rel-max', max((e, k) for k, e in errs.items()))
    for k, (shape, stride, want) in grads.items():
        assert tuple(runs[0][k].shape) == shape and errs[k] <= TOL, (k, errs[k])
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_two_sgd_steps_pick_up_in_place_updates(golden):
    """an in-place optimiser step must reach every kernel's view of the weights (the SE and FiLM kernels read the parameters themselves, the convs
    their packed images): the second step's loss follows the restatement's"""
    fx, sd = golden
    ss = _codec(golden, with_film=True).train()
    x = _wave(fx)
    strides = tuple(fx['ctor']['strides'])
    lr = 1e-3
    ref = {k: v.double().clone() for k, v in sd.items()}
    ref_losses, losses = [], []
    xd = x.to(dev())
    params = dict(ss.named_parameters())
    for step in range(3):
        p64 = {k: v.clone().requires_grad_() for k, v in ref.items()}
        l64 = F.mse_loss(R.denoising_autoencoder(p64, x.double(), True, strides), x.double())
        l64.backward()
        ref_losses.append(float(l64.detach()))
        ref = {k: (v - lr * p64[k].grad).detach() for k, v in ref.items()}
        ss.zero_grad(set_to_none=True)
        loss = F.mse_loss(_autoencode(ss, xd, True), xd)
        losses.append(float(loss.detach()))
        if step < 2:
            loss.backward()
            with torch.no_grad():
                for k in ref:
                    params[k].add_(params[k].grad, alpha=-lr)
    print('losses', losses, 'restatement', ref_losses)
    assert abs(ref_losses[1] - ref_losses[0]) > 1e-4 * ref_losses[0]      # the step moves the loss by far more than the bound below
    for got, want in zip(losses, ref_losses):
        assert abs(got - want) <= 1e-5 * abs(want), (losses, ref_losses)


def test_is_denoising_none_issues_no_film_launch(golden, monkeypatch):
    from audiolm_pytorch_amd import _lib
    fx, _ = golden
    film, plain = _codec(golden, with_film=True), _codec(golden)
    wave = fx['inputs']['wave'].to(dev())
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        none = film(wave, return_recons_only=True)
        assert not [c for c in calls if c.startswith('alm_film')] and 'alm_se_gate_fwd' in calls
        assert torch.equal(none, plain(wave, return_recons_only=True))
        assert torch.equal(film(wave, return_codes_only=True), plain(wave, return_codes_only=True))
        del calls[:]
        on = film(wave, target=wave, is_denoising=True, return_recons_only=True)
        assert calls.count('alm_film_fwd') == 2
        off = film(wave, target=wave, is_denoising=False, return_recons_only=True)
        quantized, _, _ = film(wave, target=wave, is_denoising=True, return_encoded=True)
        del calls[:]
        assert torch.equal(film.decode(quantized), film.decode(quantized)) and 'alm_film_fwd' not in calls       # decode() never applies FiLM
    assert on.shape == none.shape and not torch.equal(on, off) and not torch.equal(on, none) and not torch.equal(off, none)
    with pytest.raises(AssertionError):
        film(wave, is_denoising=True, return_recons_only=True)


def test_denoising_generator_step(golden):
    """the full training forward: the recon term is mse(target, recon) of the FiLM-conditioned codec and gradients reach both conditioners"""
    ss = _codec(golden, with_film=True, with_discriminators=True, stft_discriminator=False, multi_spectral_recon_loss_weight=0.).train()
    wave, target = rnd(2, 3840, seed=60, scale=0.3).to(dev()), rnd(2, 3840, seed=61, scale=0.3).to(dev())
    ss.rq.eval()                                                 # deterministic quantiser: the same reconstruction in every call
    total, (recon, _, _, _, _) = ss(wave, target=target, is_denoising=True, return_loss_breakdown=True)
    with torch.no_grad():
        fake = ss(wave, target=target, is_denoising=True, return_recons_only=True)
        other = ss(wave, target=target, is_denoising=False, return_recons_only=True)
    check('recon term', recon.detach().reshape(1), F.mse_loss(fake.double().cpu(), target[:, None, :].double().cpu()).reshape(1))
    assert not torch.equal(fake, other)
    total.backward()                                             # the eval-mode quantiser passes no gradient: the decoder side only
    assert ss.decoder_film.to_cond.weight.grad is not None and ss.encoder_film.to_cond.weight.grad is None
    ss.rq.train()                                                # one training step of the quantiser: its input gradient reaches the encoder side
    ss.zero_grad(set_to_none=True)
    ss(wave, target=target, is_denoising=True).backward()
    for film in (ss.encoder_film, ss.decoder_film):
        gw, gb = film.to_cond.weight.grad, film.to_cond.bias.grad
        assert gw is not None and gb is not None and bool(torch.isfinite(gw).all())
        assert float(gw[:, 0].abs().max()) > 0 and float(gw[:, 1].abs().max()) == 0 and float(gb.abs().max()) > 0
    se = ss.encoder[1][0].fn[4].net[0].weight.grad
    assert se is not None and float(se.abs().max()) > 0
