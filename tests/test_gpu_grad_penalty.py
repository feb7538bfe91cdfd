"""Gradient penalty of SoundStream training on the MI355X: the double backward through the discriminator kernels (audiolm_pytorch_amd/discriminators.py,
csrc/discr.hip alm_gconv1d_fwd_masked / alm_grad_penalty_*, csrc/stft_discr.hip alm_modrelu_bwd2 / alm_cabs_bwd2) and the discriminator branch of
SoundStream.forward with `apply_grad_penalty=True`.

Kernel level: every twice-differentiable backward (grouped conv1d, complex conv2d, STFT, ModReLU, |z|) against float64 double autograd of the same
formula on the CPU; the penalty reduction against float64.  Module level: `gradient_penalty` through MultiScaleDiscriminator and through a small
ComplexSTFTDiscriminator against the float64 restatements (tests/grad_penalty_restated.py).  End to end: the package and the total of the REAL reference
(tests/golden/soundstream_grad_penalty.pt, tests/golden/make_grad_penalty_golden.py), and SGD steps against the float64 restatement.

Tolerance (the project's convention, tests/test_gpu_stft_discr.py): the larger of 2e-5 rel-max and ten times the deviation of the SAME computation
evaluated in fp32 on the CPU from float64 -- computed here for the kernel and module cases, stored per key as `fp32_deviation` in the fixture.  The
factor ten allows for another summation order.  Every measured error is printed.  Everything is bitwise reproducible (no atomics): two runs are
torch.equal."""
import os

import pytest
import torch
import torch.nn.functional as F

import audiolm_oracle as O
import discr_restated as R
import grad_penalty_restated as GP
from common import GOLDEN_DIR, synth_state_dict
from stft_discr_restated import ComplexSTFTDiscriminatorRestated, ModReLURestated
from test_gpu_discr import CONV_CASES, GAP
from test_gpu_stft_discr import SMALL, module_pair

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
NAMES = ['scale:1', 'scale:0.5', 'scale:0.25', 'scale_grad_penalty:1', 'scale_grad_penalty:0.5', 'scale_grad_penalty:0.25', 'stft', 'stft_grad_penalty']


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def bound(ref32, ref64):
    """larger of 2e-5 and ten times the fp32-CPU deviation of this very quantity"""
    return max(TOL, 10. * relmax(ref32, ref64))


def check(name, got, ref64, ref32):
    got, ref64, ref32 = (torch.as_tensor(t).detach() for t in (got, ref64, ref32))
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if float(ref64.abs().max()) == 0.:
        assert float(got.abs().max()) == 0., name
        return
    e, tol = relmax(got, ref64), bound(ref32, ref64)
    print(f'{name}: rel-max {e:.3e} (fp32 on the CPU {relmax(ref32, ref64):.3e}, bound {tol:.3e})')
    assert e <= tol, (name, e, tol)


def leaf(t, dtype):
    """a fresh leaf of that dtype on the CPU (the caller's tensor stays as it is)"""
    return t.detach().clone().to(dtype).requires_grad_()


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def ops():
    from audiolm_pytorch_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def D():
    from audiolm_pytorch_amd import discriminators as _D
    return _D


# ---------------------------------------------------------------------------------------------- 1. grouped conv1d

def conv_inputs(B, Cin, Cout, T, k, stride, pad, groups, leaky, seed):
    x = rnd(B, Cin, T, seed=100 * seed)
    w = rnd(Cout, Cin // groups, k, seed=100 * seed + 1, scale=(Cin // groups * k) ** -0.5)
    b = rnd(Cout, seed=100 * seed + 2, scale=0.1)
    Tout = (T + 2 * pad - k) // stride + 1
    return x, w, b, rnd(B, Cout, Tout, seed=100 * seed + 3), rnd(B, Cin, T, seed=100 * seed + 4)


def conv_double_ref(x, w, b, g, v, stride, pad, groups, leaky, dtype):
    """dx with create_graph, S = <v, dx>, then dS/dg and dS/dw, by CPU autograd"""
    x, w, b, g = (leaf(t, dtype) for t in (x, w, b, g))
    pre = F.conv1d(x, w, b, stride=stride, padding=pad, groups=groups)
    y = F.leaky_relu(pre, 0.1) if leaky else pre
    dx, = torch.autograd.grad(y, x, g, create_graph=True)
    dg, dw = torch.autograd.grad((dx * v.to(dtype)).sum(), (g, w))
    return (dx.detach(), dg, dw), float(pre.detach().abs().min())


@pytest.mark.parametrize('B,Cin,Cout,T,k,stride,pad,groups,leaky,seed', CONV_CASES)
def test_conv_double_backward(ops, D, B, Cin, Cout, T, k, stride, pad, groups, leaky, seed):
    x, w, b, g, v = conv_inputs(B, Cin, Cout, T, k, stride, pad, groups, leaky, seed)
    r64, gap = conv_double_ref(x, w, b, g, v, stride, pad, groups, leaky, F64)
    r32, _ = conv_double_ref(x, w, b, g, v, stride, pad, groups, leaky, F32)
    assert not leaky or gap > GAP, f'a pre-activation lies {gap:.3g} from the LeakyReLU kink: choose another seed'
    vd = v.to(dev())

    def run():
        xd, wd, bd, gd = (t.to(dev()).requires_grad_() for t in (x, w, b, g))
        y = D._GConv1dFn.apply(xd, wd, bd, stride, pad, groups, leaky)
        dx, = torch.autograd.grad(y, xd, gd, create_graph=True)
        dg, dw = torch.autograd.grad((dx * vd).sum(), (gd, wd))
        assert dg.grad_fn is None and dw.grad_fn is None
        masked = ops.gconv1d_fwd_masked(vd, wd.detach(), y.detach() if leaky else None, stride=stride, padding=pad, groups=groups)
        return dx.detach(), dg, dw, masked

    got = run()
    for name, a, c, d in zip(('dx', 'dS/dg', 'dS/dw'), got, r64, r32):
        check(name, a, c, d)
    assert torch.equal(got[3], got[1]), 'the direct launch of alm_gconv1d_fwd_masked differs from the autograd path'
    assert same(got, run()), 'two runs differ'


# ---------------------------------------------------------------------------------------------- 2. the penalty reduction

def penalty_ref(G, weight, center, dtype):
    G = leaf(G, dtype)
    out = weight * ((torch.linalg.vector_norm(G, dim=1) - center) ** 2).mean()
    (out * 1.7).backward()
    return out.detach().reshape(1), G.grad


@pytest.mark.parametrize('center', [0., 1.])
@pytest.mark.parametrize('rows,n,zero_row', [(1, 1, None), (4, 301, 2), (2, 1283, None), (3, 70001, 1), (2, 17, 0)])
def test_penalty_reduction(ops, D, rows, n, zero_row, center):
    G = rnd(rows, n, seed=40 + rows, scale=0.05)
    if zero_row is not None:
        G[zero_row] = 0.
    r64, r32 = penalty_ref(G, 10., center, F64), penalty_ref(G, 10., center, F32)

    def run():
        Gd = G.to(dev()).requires_grad_()
        out = D.penalty_of_gradients(Gd, 10., center)
        (out * 1.7).backward()
        return out.detach().reshape(1), Gd.grad

    got = run()
    check('penalty', got[0], r64[0], r32[0])
    check('d penalty / dG', got[1], r64[1], r32[1])
    if zero_row is not None:
        assert float(got[1][zero_row].abs().max()) == 0. and bool(torch.isfinite(got[1]).all())
    assert same(got, run()), 'two runs differ'
    with torch.no_grad():                                        # without a graph: the forward launches only, the same value
        assert torch.equal(D.penalty_of_gradients(G.to(dev()), 10., center).reshape(1), got[0])


# ---------------------------------------------------------------------------------------------- 3. ModReLU and |z|, second order

def modrelu_double_ref(z, b, g, v, beta, dtype):
    m = ModReLURestated().to(dtype)
    m.b.data.fill_(b)
    z, g = leaf(z, dtype), leaf(g, dtype)
    y = torch.view_as_real(m(torch.view_as_complex(z)))
    dz, db = torch.autograd.grad(y, (z, m.b), g, create_graph=True)
    d2 = torch.autograd.grad((dz * v.to(dtype)).sum() + beta * db, (g, z, m.b))
    return dz.detach(), db.detach(), *d2


def abs_double_ref(z, g, v, dtype):
    z, g = leaf(z, dtype), leaf(g, dtype)
    dz, = torch.autograd.grad(torch.view_as_complex(z).abs(), z, g, create_graph=True)
    return dz.detach(), *torch.autograd.grad((dz * v.to(dtype)).sum(), (g, z))


# (2, 3, 5, 7): 210 pairs, no multiple of 256; 3000 pairs: several waves' worth, no multiple of 256; 8200 pairs: more than one 4096-pair block span
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (3, 1000), (2, 4100)])
@pytest.mark.parametrize('b', [-0.2, 0.3])
def test_modrelu_and_abs_second_order(D, shape, b):
    z = rnd(*shape, 2, seed=51, scale=0.3)
    g, v, ga, beta = rnd(*shape, 2, seed=52), rnd(*shape, 2, seed=53), rnd(*shape, seed=54), 0.7
    mod = z.double().pow(2).sum(-1).sqrt()
    assert float((mod + b).abs().min()) > 1e-5 and float(mod.min()) > 1e-5      # the seed keeps every |z| + b and |z| away from its kink
    inactive = int((mod + b <= 0).sum())
    assert (inactive > 0) == (b < 0), inactive                   # a negative b switches units off
    r64, r32 = modrelu_double_ref(z, b, g, v, beta, F64), modrelu_double_ref(z, b, g, v, beta, F32)
    vd = v.to(dev())

    def run():
        zd, gd, bd = z.to(dev()).requires_grad_(), g.to(dev()).requires_grad_(), torch.tensor(b, device=dev(), requires_grad=True)
        y = D._ModReLUFn.apply(zd, bd)
        dz, db = torch.autograd.grad(y, (zd, bd), gd, create_graph=True)
        d2 = torch.autograd.grad((dz * vd).sum() + beta * db, (gd, zd, bd))
        return dz.detach(), db.detach(), *d2

    got = run()
    for name, a, c, d in zip(('dz', 'db', 'dS/dg', 'dS/dz', 'dS/db'), got, r64, r32):
        check(f'modrelu {name}', a, c, d)
    assert same(got, run()), 'two runs differ'

    a64, a32 = abs_double_ref(z, ga, v, F64), abs_double_ref(z, ga, v, F32)

    def run_abs():
        zd, gd = z.to(dev()).requires_grad_(), ga.to(dev()).requires_grad_()
        dz, = torch.autograd.grad(D._CAbsFn.apply(zd), zd, gd, create_graph=True)
        return dz.detach(), *torch.autograd.grad((dz * vd).sum(), (gd, zd))

    got = run_abs()
    for name, a, c, d in zip(('dz', 'dS/dg', 'dS/dz'), got, a64, a32):
        check(f'|z| {name}', a, c, d)
    assert same(got, run_abs()), 'two runs differ'


def test_second_order_at_zero(ops):
    """at z = 0 the backward passes are dz = 0, db += g_re (ModReLU, active) and dz = 0 (|z|): as functions their derivatives are (beta, 0) for g and
    nothing else -- finite, no division by zero"""
    z = torch.zeros(3, 2, device=dev())
    z[1] = torch.tensor([0.3, -0.4])
    g, v = rnd(3, 2, seed=55).to(dev()), rnd(3, 2, seed=56).to(dev())
    beta = torch.tensor(0.7, device=dev())
    dg, dz, db = ops.modrelu_bwd2(g, z, torch.tensor(0.25, device=dev()), v, beta)
    assert dg[0].tolist() == [float(beta), 0.] and dg[2].tolist() == [float(beta), 0.] and dz[0].tolist() == [0., 0.]
    assert bool(torch.isfinite(dg).all() and torch.isfinite(dz).all() and torch.isfinite(db))
    dg, dz = ops.complex_abs_bwd2(g[:, 0].contiguous(), z, v)
    assert float(dg[0]) == 0. and dz[0].tolist() == [0., 0.] and bool(torch.isfinite(dg).all() and torch.isfinite(dz).all())


# ---------------------------------------------------------------------------------------------- 4. complex conv2d and STFT

def cconv_double_ref(x, w, b, g, v, stride, padding, residual, dtype):
    x, w, b, g = (leaf(t, dtype) for t in (x, w, b, g))
    xc = torch.view_as_complex(x)
    y = F.conv2d(xc, torch.view_as_complex(w), torch.view_as_complex(b), stride=stride, padding=padding)
    y = torch.view_as_real(y + xc if residual else y)
    dx, = torch.autograd.grad(y, x, g, create_graph=True)
    return dx.detach(), *torch.autograd.grad((dx * v.to(dtype)).sum(), (g, w))


# (B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw, residual): a strided layer of the small module, the second conv of a residual unit, the final conv
@pytest.mark.parametrize('B,Cin,Cout,H,W,kh,kw,sh,sw,ph,pw,residual', [(2, 4, 8, 33, 21, 3, 4, 1, 2, 1, 2, False), (2, 4, 4, 33, 21, 3, 3, 1, 1, 1, 1, True),
                                                                        (2, 8, 8, 17, 6, 4, 4, 2, 2, 2, 2, False), (1, 8, 1, 17, 6, 16, 1, 1, 1, 0, 0, False)])
def test_complex_conv_double_backward(D, B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw, residual):
    x, w, b = rnd(B, Cin, H, W, 2, seed=5), rnd(Cout, Cin, kh, kw, 2, seed=6, scale=(Cin * kh * kw) ** -0.5), rnd(Cout, 2, seed=7, scale=0.1)
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    g, v = rnd(B, Cout, Ho, Wo, 2, seed=8), rnd(B, Cin, H, W, 2, seed=9)
    r64 = cconv_double_ref(x, w, b, g, v, (sh, sw), (ph, pw), residual, F64)
    r32 = cconv_double_ref(x, w, b, g, v, (sh, sw), (ph, pw), residual, F32)
    vd = v.to(dev())

    def run():
        xd, wd, bd, gd = (t.to(dev()).requires_grad_() for t in (x, w, b, g))
        y = D._CConv2dFn.apply(xd, wd, bd, xd if residual else None, (sh, sw), (ph, pw))
        dx, = torch.autograd.grad(y, xd, gd, create_graph=True)
        return dx.detach(), *torch.autograd.grad((dx * vd).sum(), (gd, wd))

    got = run()
    for name, a, c, d in zip(('dx', 'dS/dg', 'dS/dw'), got, r64, r32):
        check(name, a, c, d)
    assert same(got, run()), 'two runs differ'


def stft_double_ref(x, g, v, n_fft, hop, win, normalized, dtype):
    x, g = leaf(x, dtype), leaf(g, dtype)
    X = torch.view_as_real(torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win).to(dtype), normalized=normalized,
                                      return_complex=True))
    dx, = torch.autograd.grad(X, x, g, create_graph=True)
    return dx.detach(), torch.autograd.grad((dx * v.to(dtype)).sum(), g)[0]


@pytest.mark.parametrize('B,n,n_fft,hop,win,normalized', [(2, 2560, 1024, 256, 1024, False), (3, 331, 64, 16, 48, False), (2, 100, 32, 5, 32, True)])
def test_stft_double_backward(ops, D, B, n, n_fft, hop, win, normalized):
    x, g, v = rnd(B, n, seed=3, scale=0.5), rnd(B, n_fft // 2 + 1, n // hop + 1, 2, seed=4), rnd(B, n, seed=5)
    r64, r32 = stft_double_ref(x, g, v, n_fft, hop, win, normalized, F64), stft_double_ref(x, g, v, n_fft, hop, win, normalized, F32)
    basis = ops.stft_basis(n_fft, torch.hann_window(win), normalized, dev())
    vd = v.to(dev())

    def run():
        xd, gd = x.to(dev()).requires_grad_(), g.to(dev()).requires_grad_()
        dx, = torch.autograd.grad(D._StftFn.apply(xd, basis, n_fft, hop), xd, gd, create_graph=True)
        return dx.detach(), torch.autograd.grad((dx * vd).sum(), gd)[0]

    got = run()
    check('dx', got[0], r64[0], r32[0])
    check('dS/dg', got[1], r64[1], r32[1])
    assert same(got, run()), 'two runs differ'


# ---------------------------------------------------------------------------------------------- 5. whole discriminators

def penalty_through(module, wave, dtype):
    """(penalty, parameter gradients) of gradient_penalty(wave, module(wave)) by CPU autograd, and what lies near a kink"""
    module = module.to(dtype)
    module.zero_grad(set_to_none=True)
    x = leaf(wave, dtype)
    pen = GP.gradient_penalty(x, module(x))
    pen.backward()
    return pen.detach().reshape(1), {k: p.grad for k, p in module.named_parameters()}


def compare_module(name, ours, wave, r64, r32, D):
    def run():
        ours.zero_grad(set_to_none=True)
        x = wave.to(dev()).requires_grad_()
        pen = D.gradient_penalty(x, ours(x))
        pen.backward()
        return [pen.detach().reshape(1), *(p.grad for p in ours.parameters())]

    got = run()
    check(f'{name} penalty', got[0], r64[0], r32[0])
    for (k, p), gr in zip(ours.named_parameters(), got[1:]):
        want64, want32 = r64[1][k], r32[1][k]
        if want64 is None or float(want64.abs().max()) == 0.:    # a bias ahead of a piecewise-linear unit: no gradient, or exact zeros
            assert gr is None or float(gr.abs().max()) == 0., k
        else:
            assert gr is not None and gr.grad_fn is None, k
            check(f'{name} d {k}', gr, want64, want32)
    assert same(got, run()), 'two runs differ'


@pytest.mark.parametrize('T', [1000, 1283])
def test_penalty_through_the_wave_discriminator(D, T):
    import audiolm_pytorch_amd as A
    torch.manual_seed(60)
    ours = A.MultiScaleDiscriminator()
    ref = R.MultiScaleDiscriminatorRestated()
    ref.load_state_dict(ours.state_dict(), strict=True)
    wave = rnd(2, 1, T, seed=63, scale=0.3)                   # seed 61 puts one pre-activation 6.3e-8 from zero, within ten fp32 errors
    (pre64, r64), (pre32, r32) = (R.leaky_inputs(ref, lambda dt=dt: penalty_through(ref, wave, dt)) for dt in (F64, F32))
    v64, v32 = (torch.cat([t.double().reshape(-1) for t in pre]) for pre in (pre64, pre32))
    unsafe = int((v64.abs() <= 10. * (v32 - v64).abs()).sum())
    print(f'T = {T}: {v64.numel()} LeakyReLU pre-activations, the nearest {float(v64.abs().min()):.3e} from zero, {unsafe} within ten fp32 errors')
    assert unsafe == 0, 'choose another seed'
    compare_module(f'T = {T}', ours.to(dev()), wave, r64, r32, D)


def test_penalty_through_the_stft_discriminator(D):
    ours, ref = module_pair(SMALL, True, seed=23)
    wave = rnd(2, 1, 2560, seed=62, scale=0.3)
    pres = []
    for dt in (F64, F32):
        ref.to(dt).probe(True)
        out = penalty_through(ref, wave, dt)
        pres.append((ref.pre_activations().double(), ref.complex_logits.abs().double().reshape(-1), out))
        ref.probe(False)
    (p64, l64, r64), (p32, l32, r32) = pres
    unsafe = int((p64.abs() <= 10. * (p32 - p64).abs()).sum()) + int((l64 <= 10. * (l32 - l64).abs()).sum())
    print(f'{p64.numel()} ModReLU pre-activations, the nearest {float(p64.abs().min()):.3e} from zero; |logit| >= {float(l64.min()):.3e}; {unsafe} unsafe')
    assert unsafe == 0, 'choose another seed'
    compare_module('stft', ours, wave, r64, r32, D)


# ---------------------------------------------------------------------------------------------- 6. SoundStream against the real reference

@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_grad_penalty.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def _soundstream(golden, stft=True, penalty=True):
    import audiolm_pytorch_amd as A
    fx, sd = golden
    ss = A.SoundStream(**fx['ctor'], stft_discriminator=stft, with_discriminators=True, with_grad_penalty=penalty)
    ss.load_state_dict(sd if stft else {k: v for k, v in sd.items() if not k.startswith('stft_discriminator.')}, strict=True)
    ss.to(dev()).train()
    ss.rq.eval()                                                 # deterministic quantiser, like the maker
    return ss


def _key_tol(fx, key):
    return max(TOL, 10. * fx['fp32_deviation'][key])


def _discr_grads(ss):
    out = {k: (None if p.grad is None else p.grad.clone()) for k, p in ss.named_parameters() if k.startswith(('discriminators.', 'stft_discriminator.'))}
    assert all(p.grad is None for k, p in ss.named_parameters() if not k.startswith(('discriminators.', 'stft_discriminator.'))), 'a codec gradient'
    ss.zero_grad(set_to_none=True)
    return out


def _digest_check(fx, tag, grads, digests):
    worst = 0.
    for k, d in digests.items():
        if d is None or d['norm'] == 0.:                         # untouched by this entry, or the exact zeros torch gives a bias ahead of a LeakyReLU
            assert grads[k] is None or float(grads[k].abs().max()) == 0., (tag, k)
            continue
        assert grads[k] is not None and grads[k].grad_fn is None, (tag, k)
        tol = _key_tol(fx, f'{tag}:{k}')
        flat = grads[k].detach().float().reshape(-1).cpu()
        e = max(relmax(flat[::d['stride']], d['sample']), abs(float(flat.double().norm()) - d['norm']) / d['norm'])
        worst = max(worst, e)
        if e > 0.5 * tol:
            print(f'{tag} {k}: digest deviation {e:.3e} (bound {tol:.3e})')
        assert e <= tol, (tag, k, e, tol)
    print(f'{tag}: worst gradient digest deviation {worst:.3e} over {len(digests)} tensors')


def _check_loss(fx, key, got, ref):
    e, tol = relmax(got.detach().reshape(1), ref.reshape(1)), _key_tol(fx, key)
    print(f'{key}: {float(got.detach()):.9g} against {float(ref):.9g}: rel {e:.3e} (bound {tol:.3e})')
    assert e <= tol, (key, e, tol)


def _package(ss, wave):
    """the trainer's loop: one backward(retain_graph=True) per entry; gradients zeroed between entries, like the maker"""
    ss.zero_grad(set_to_none=True)
    pkg = ss(wave, return_discr_loss=True, return_discr_losses_separately=True, apply_grad_penalty=True)
    grads = {}
    for name, loss in pkg:
        loss.backward(retain_graph=True)
        grads[name] = _discr_grads(ss)
    return [(n, v.detach()) for n, v in pkg], grads


def test_package_matches_the_reference(golden, D):
    fx, _ = golden
    ss = _soundstream(golden)
    wave = fx['inputs']['wave'].to(dev())
    pkg, grads = _package(ss, wave)
    assert [n for n, _ in pkg] == [n for n, _ in fx['outputs']['separately']] == NAMES
    for (n, got), (_, ref) in zip(pkg, fx['outputs']['separately']):
        _check_loss(fx, f'separately:{n}', got, ref)
    for n in NAMES:
        _digest_check(fx, f'entry:{n}', grads[n], fx['outputs']['entry_grads'][n])
    # the reference's labels: the scales zipped with the flat [real, fake] list, so 'scale_grad_penalty:0.5' is the FAKE penalty at scale 1
    b = wave.shape[0]
    both = torch.cat((wave[:, None], ss(wave, return_recons_only=True).detach()), dim=0).requires_grad_()
    logits = ss.discriminators[0](both)
    gradients = D.wave_gradients(both, D.hinge_discr_loss(logits[b:], logits[:b]))
    byname = dict(pkg)
    assert torch.equal(D.penalty_of_gradients(gradients[:b]).detach(), byname['scale_grad_penalty:1'])
    assert torch.equal(D.penalty_of_gradients(gradients[b:]).detach(), byname['scale_grad_penalty:0.5'])
    # determinism: the same loop again, everything bitwise the first's
    pkg2, grads2 = _package(ss, wave)
    assert all(torch.equal(a, c) for (_, a), (_, c) in zip(pkg, pkg2))
    differ = [(n, k) for n in NAMES for k in grads[n] if not same([grads[n][k]], [grads2[n][k]])]
    assert not differ, differ


def test_total_matches_the_reference(golden):
    fx, _ = golden
    ss = _soundstream(golden)
    wave = fx['inputs']['wave'].to(dev())
    ss.zero_grad(set_to_none=True)
    total = ss(wave, return_discr_loss=True, apply_grad_penalty=True)
    total.backward()
    grads = _discr_grads(ss)
    _check_loss(fx, 'loss:total', total, fx['outputs']['total'])
    _digest_check(fx, 'total', grads, fx['outputs']['total_grads'])
    with torch.no_grad():
        plain = dict(ss(wave, return_discr_loss=True, return_discr_losses_separately=True))
    pkg = dict(ss(wave, return_discr_loss=True, return_discr_losses_separately=True, apply_grad_penalty=True))
    scales = torch.stack([plain[n] for n in NAMES[:3]]).mean()
    assert torch.equal(total.detach(), (scales + plain['stft'] + pkg['stft_grad_penalty']).detach())
    # nothing from a wave penalty reaches discriminators.*: their gradients are those of the call without the penalty, bit for bit
    ss.zero_grad(set_to_none=True)
    ss(wave, return_discr_loss=True).backward()
    without = _discr_grads(ss)
    assert all(torch.equal(grads[k], without[k]) for k in grads if k.startswith('discriminators.'))
    assert any(not torch.equal(grads[k], without[k]) for k in grads if k.startswith('stft_discriminator.'))


def test_without_an_stft_discriminator(golden):
    fx, _ = golden
    ss = _soundstream(golden, stft=False)
    wave = fx['inputs']['wave'].to(dev())
    pkg, grads = _package(ss, wave)
    assert [n for n, _ in pkg] == NAMES[:6]
    for (n, got), (_, ref) in zip(pkg, fx['outputs']['separately']):
        _check_loss(fx, f'separately:{n}', got, ref)               # the wave discriminators do not depend on the STFT one
    ss.zero_grad(set_to_none=True)
    total = ss(wave, return_discr_loss=True, apply_grad_penalty=True)
    assert torch.equal(total.detach(), torch.stack([v for _, v in pkg[:3]]).mean())


# ---------------------------------------------------------------------------------------------- 7. unchanged behaviour

def test_the_switch_changes_nothing_else(golden, monkeypatch):
    from audiolm_pytorch_amd import ops as _ops
    fx, _ = golden
    wave = fx['inputs']['wave'].to(dev())
    second_order = []
    for name in ('gconv1d_fwd_masked', 'modrelu_bwd2', 'complex_abs_bwd2', 'grad_penalty', 'grad_penalty_bwd'):
        monkeypatch.setattr(_ops, name, lambda *a, _n=name, **k: second_order.append(_n))
    results = []
    for penalty in (True, False):
        ss = _soundstream(golden, penalty=penalty)
        ss.zero_grad(set_to_none=True)
        loss = ss(wave, return_discr_loss=True)
        loss.backward()
        assert all(p.grad is None or p.grad.grad_fn is None for p in ss.parameters())      # a plain backward records nothing
        grads = _discr_grads(ss)
        gen = ss(wave)
        if penalty:                                              # the generator branch accepts the flag and ignores it, like the reference
            assert torch.equal(ss(wave, apply_grad_penalty=True).detach(), gen.detach())
        gen.backward()
        results.append((loss.detach(), grads, gen.detach(), {k: p.grad for k, p in ss.named_parameters() if p.grad is not None}))
        with torch.no_grad():
            results[-1] += (ss(wave, return_discr_loss=True, return_discr_losses_separately=True),)
    (l1, g1, t1, q1, s1), (l2, g2, t2, q2, s2) = results
    assert torch.equal(l1, l2) and torch.equal(t1, t2) and g1.keys() == g2.keys() and q1.keys() == q2.keys()
    assert all(same([g1[k]], [g2[k]]) for k in g1) and all(torch.equal(q1[k], q2[k]) for k in q1)
    assert [n for n, _ in s1] == [n for n, _ in s2] and all(torch.equal(a, c) for (_, a), (_, c) in zip(s1, s2))
    assert not second_order, second_order                        # no second-order kernel without apply_grad_penalty


# ---------------------------------------------------------------------------------------------- 8. refusals

def test_what_is_not_twice_differentiable_raises_by_name(D):
    conv = torch.nn.Conv1d(8, 16, 5, stride=2, padding=2, groups=2).to(dev())
    x = rnd(2, 8, 37, seed=9).to(dev()).requires_grad_()
    dw, = torch.autograd.grad(D.conv1d_act(conv, x, leaky=True).sum(), conv.weight, create_graph=True)
    with pytest.raises(NotImplementedError, match='gconv1d_wgrad'):
        dw.sum().backward()
    a, b = rnd(3, 50, seed=70).to(dev()).requires_grad_(), rnd(3, 50, seed=71).to(dev())
    da, = torch.autograd.grad(D.mse_loss(a, b), a, create_graph=True)
    with pytest.raises(NotImplementedError, match='squared-error'):
        da.sum().backward()
    pool = D.AvgPoolDownsample(2)
    gp = rnd(2, 8, 19, seed=75).to(dev()).requires_grad_()      # the pooling backward depends on its incoming gradient alone
    dx, = torch.autograd.grad(pool(x), x, gp, create_graph=True)
    with pytest.raises(NotImplementedError, match='avgpool1d_bwd'):
        dx.sum().backward()
    w = torch.nn.Parameter(rnd(4, 2, 3, 3, 2, seed=72).to(dev()))
    z = rnd(1, 2, 9, 9, 2, seed=73).to(dev()).requires_grad_()
    dcw, = torch.autograd.grad(D._CConv2dFn.apply(z, w, torch.zeros(4, 2, device=dev()), None, 1, 1).sum(), w, create_graph=True)
    with pytest.raises(NotImplementedError, match='cconv2d_wgrad'):
        dcw.sum().backward()
    # and nothing is differentiable a third time: the second-order results carry an error node, not a silent constant
    g = rnd(2, 16, 19, seed=74).to(dev()).requires_grad_()
    dx, = torch.autograd.grad(D.conv1d_act(conv, x, leaky=True), x, g, create_graph=True)
    vv = rnd(2, 8, 37, seed=76).to(dev()).requires_grad_()
    dg, = torch.autograd.grad((dx * vv).sum(), g, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        dg.sum().backward()


# ---------------------------------------------------------------------------------------------- 9. SGD with the penalty on every step

def test_sgd_steps_with_the_penalty_follow_the_float64_restatement(golden):
    """three plain SGD steps of the discriminators in place, the penalty on every step: every loss follows the float64 restatement, so the double
    backward reads the parameters' current values.  The step size: the same loop in fp32 on the CPU leaves float64 by 1.5e-4 of the loss after three steps
    at lr 2e-4 and by 1.3e-5 at 2e-5 (units cross their kinks as the parameters move; measured with a stand-in fake wave), so lr 5e-6 keeps that
    floor near 3e-6, under the fixture's 2e-5, while three steps still move the loss by about 2 %, a thousand times the tolerance"""
    fx, sd = golden
    ss = _soundstream(golden)
    wave = fx['inputs']['wave']
    xd = wave.to(dev())
    with torch.no_grad():
        quantized = ss(xd, return_encoded=True)[0]               # the eval-mode quantiser and the decoder stay fixed: one fake wave for the whole test
    dec = {k: v.double() for k, v in sd.items() if k.startswith('decoder.')}
    fake64 = O.soundstream_decoder(dec, quantized.double().cpu().transpose(1, 2), strides=(2, 4, 5, 8)).detach()
    real64 = wave.double()[:, None, :]
    discrs = [R.MultiScaleDiscriminatorRestated().double() for _ in range(3)]
    for i, d in enumerate(discrs):
        d.load_state_dict({k[len(f'discriminators.{i}.'):]: v.double() for k, v in sd.items() if k.startswith(f'discriminators.{i}.')}, strict=True)
    stft = ComplexSTFTDiscriminatorRestated()
    stft.load_state_dict({k[len('stft_discriminator.'):]: v for k, v in sd.items() if k.startswith('stft_discriminator.')}, strict=True)
    stft.double()
    d_params = [*(p for d in discrs for p in d.parameters()), *stft.parameters()]
    ours = [*ss.discriminators.parameters(), *ss.stft_discriminator.parameters()]
    lr = 5e-6

    def ref_loss():
        return GP.discr_losses_with_penalty(discrs, (None, 2, 2), ss.discr_multi_scales, stft, real64, fake64, package=False)[0]

    got, want = [], []
    for _ in range(3):
        for p in d_params:
            p.grad = None
        loss64 = ref_loss()
        loss64.backward()
        ss.zero_grad(set_to_none=True)
        loss = ss(xd, return_discr_loss=True, apply_grad_penalty=True)
        loss.backward()
        with torch.no_grad():
            for p in d_params:
                if p.grad is not None:
                    p.add_(p.grad, alpha=-lr)
            for p in ours:
                if p.grad is not None:
                    p.add_(p.grad, alpha=-lr)
        want.append(float(loss64.detach()))
        got.append(float(loss.detach()))
    want.append(float(ref_loss().detach()))
    got.append(float(ss(xd, return_discr_loss=True, apply_grad_penalty=True).detach()))
    print('discriminator loss with the penalty per step:', got, 'float64:', want)
    assert want[0] - want[-1] > 500 * TOL * want[0], 'the steps are too small to show anything'
    tol = _key_tol(fx, 'loss:total')
    for a, c in zip(got, want):
        assert abs(a - c) <= tol * abs(c), (got, want)
