"""ComplexSTFTDiscriminator of SoundStream training on the MI355X (csrc/stft_discr.hip, audiolm_pytorch_amd/discriminators.py, the loss branches of
soundstream.py).

Op level: the STFT against float64 torch.stft autograd, the complex conv2d (y / dx / dW / db) against float64 complex F.conv2d autograd, ModReLU and
|z| against the float64 formula through torch autograd, the complex L1 mean against float64 F.l1_loss.  Module: ComplexSTFTDiscriminator at its defaults
and at the smallest geometry its 16-row final conv admits against the float64 restatement of tests/stft_discr_restated.py.  End to end: the loss
branches of SoundStream.forward against the REAL reference (tests/golden/soundstream_losses_stft.pt, tests/golden/make_stft_discr_golden.py), an
instance handed in against `stft_discriminator=True`, SGD steps against the float64 restatement.

Tolerance: op and module level, the larger of 2e-5 rel-max (the project's fp32 conv tolerance, tests/test_gpu_discr.py) and ten times the deviation of
the same case evaluated in fp32 on the CPU from float64 (computed here; the factor ten allows for another summation order and a DFT-as-GEMM versus an
FFT).  For the fixture, per key the larger of 2e-5 and ten times that key's stored fp32 deviation.  Every measured error is printed.  Every op and the
end-to-end gradients are bitwise reproducible (no atomics): two runs are torch.equal."""
import os

import pytest
import torch
import torch.nn.functional as F

import audiolm_oracle as O
import discr_restated as R
from common import GOLDEN_DIR, synth_state_dict
from stft_discr_restated import ComplexSTFTDiscriminatorRestated

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
SMALL = dict(channels=4, strides=((1, 2), (2, 2)), chan_mults=(1, 2), n_fft=64, hop_length=16, win_length=64)


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
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    e, tol = relmax(got, ref64), bound(ref32, ref64)
    print(f'{name}: rel-max {e:.3e} (fp32 on the CPU {relmax(ref32, ref64):.3e}, bound {tol:.3e})')
    assert e <= tol, (name, e, tol)


@pytest.fixture(scope='module')
def ops():
    from audiolm_pytorch_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------- STFT

# (B, n, n_fft, hop, win, normalized): the module's defaults, the shortest legal clip, a window shorter than n_fft with n no multiple of hop, hop not
# dividing n_fft
STFT_CASES = [(2, 2560, 1024, 256, 1024, False), (1, 513, 1024, 256, 1024, False), (3, 331, 64, 16, 48, False), (2, 100, 32, 5, 32, True)]


def stft_ref(x, G, n_fft, hop, win, normalized, dtype):
    x = x.detach().clone().to(dtype).requires_grad_()
    X = torch.view_as_real(torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win).to(dtype), normalized=normalized,
                                      return_complex=True))
    (X * G.to(dtype)).sum().backward()
    return X.detach(), x.grad


@pytest.mark.parametrize('B,n,n_fft,hop,win,normalized', STFT_CASES)
def test_stft_forward_backward(ops, B, n, n_fft, hop, win, normalized):
    x = rnd(B, n, seed=3, scale=0.5)
    T, Fq = n // hop + 1, n_fft // 2 + 1
    assert ops.stft_frames(n, n_fft, hop) == T
    G = rnd(B, Fq, T, 2, seed=4)
    X64, dx64 = stft_ref(x, G, n_fft, hop, win, normalized, F64)
    X32, dx32 = stft_ref(x, G, n_fft, hop, win, normalized, F32)
    basis = ops.stft_basis(n_fft, torch.hann_window(win), normalized, dev())
    X = ops.stft(x.to(dev()), basis, n_fft, hop)
    dx = ops.stft_bwd(G.to(dev()), basis, n, n_fft, hop)
    check('X', X, X64, X32)
    check('dx', dx, dx64, dx32)
    assert torch.equal(X, ops.stft(x.to(dev()), basis, n_fft, hop)) and torch.equal(dx, ops.stft_bwd(G.to(dev()), basis, n, n_fft, hop))


def test_stft_refuses_a_clip_the_reflection_cannot_pad(ops):
    from audiolm_pytorch_amd import _lib
    basis = ops.stft_basis(1024, torch.hann_window(1024), False, dev())
    with pytest.raises(_lib.AlmError):
        ops.stft(torch.zeros(1, 512, device=dev()), basis, 1024, 256)
    X = torch.zeros(1, 513, 3, 2, device=dev())
    with pytest.raises(_lib.AlmError, match='UNSUPPORTED'):
        _lib.call('alm_stft_fwd', X.data_ptr(), basis.data_ptr(), X.data_ptr(), 1, 512, 1024, 256, 513, None)


# ---------------------------------------------------------------------------------------------- complex conv2d

# (B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw): every layer form of the module at its defaults and at small settings, widths 1 and 2 (narrower than the
# kernel), channel counts that are no multiple of the tile
CCONV_CASES = [(2, 1, 32, 37, 11, 7, 7, 1, 1, 3, 3), (2, 32, 32, 19, 6, 3, 3, 1, 1, 1, 1), (2, 32, 64, 19, 6, 3, 4, 1, 2, 1, 2),
               (2, 64, 128, 19, 4, 4, 4, 2, 2, 2, 2), (2, 256, 256, 9, 2, 3, 3, 1, 1, 1, 1), (1, 256, 256, 9, 1, 4, 4, 2, 2, 2, 2),
               (2, 256, 1, 65, 2, 16, 1, 1, 1, 0, 0), (2, 4, 8, 33, 21, 3, 4, 1, 2, 1, 2), (1, 8, 1, 17, 6, 16, 1, 1, 1, 0, 0)]


def cconv_ref(x, w, b, G, stride, padding, dtype):
    x, w, b = (t.detach().clone().to(dtype).requires_grad_() for t in (x, w, b))
    y = torch.view_as_real(F.conv2d(torch.view_as_complex(x), torch.view_as_complex(w), torch.view_as_complex(b), stride=stride, padding=padding))
    (y * G.to(dtype)).sum().backward()
    return y.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize('B,Cin,Cout,H,W,kh,kw,sh,sw,ph,pw', CCONV_CASES)
def test_complex_conv_forward_backward(ops, B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw):
    fan = (Cin * kh * kw) ** -0.5
    x, w, b = rnd(B, Cin, H, W, 2, seed=5), rnd(Cout, Cin, kh, kw, 2, seed=6, scale=fan), rnd(Cout, 2, seed=7, scale=0.1)
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    assert ops.cconv2d_out_hw(H, W, (kh, kw), (sh, sw), (ph, pw)) == (Ho, Wo)
    G = rnd(B, Cout, Ho, Wo, 2, seed=8)
    r64 = cconv_ref(x, w, b, G, (sh, sw), (ph, pw), F64)
    r32 = cconv_ref(x, w, b, G, (sh, sw), (ph, pw), F32)
    xd, wd, bd, Gd = (t.to(dev()) for t in (x, w, b, G))

    def run():
        y = ops.cconv2d(xd, wd, bd, stride=(sh, sw), padding=(ph, pw))
        dx = ops.cconv2d_dgrad(Gd, wd, H, W, stride=(sh, sw), padding=(ph, pw))
        dw, db = ops.cconv2d_wgrad(Gd, xd, (kh, kw), stride=(sh, sw), padding=(ph, pw))
        return y, dx, dw, db

    got = run()
    for name, g, a, c in zip(('y', 'dx', 'dw', 'db'), got, r64, r32):
        check(name, g, a, c)
    res = rnd(B, Cout, Ho, Wo, 2, seed=9).to(dev())
    yr = ops.cconv2d(xd, wd, bd, stride=(sh, sw), padding=(ph, pw), residual=res)
    check('y + residual', yr, r64[0] + res.double().cpu(), r32[0] + res.cpu())
    assert all(torch.equal(a, c) for a, c in zip(got, run()))


# ---------------------------------------------------------------------------------------------- ModReLU, |z|, complex L1

def modrelu_ref(z, b, G, dtype):
    z, b = z.detach().clone().to(dtype).requires_grad_(), torch.tensor(b, dtype=dtype, requires_grad=True)
    zc = torch.view_as_complex(z)
    y = torch.view_as_real(F.relu(torch.abs(zc) + b) * torch.exp(1.j * torch.angle(zc)))
    (y * G.to(dtype)).sum().backward()
    return y.detach(), z.grad, b.grad


def abs_ref(z, G, dtype):
    z = z.detach().clone().to(dtype).requires_grad_()
    y = torch.view_as_complex(z).abs()
    (y * G.to(dtype)).sum().backward()
    return y.detach(), z.grad


def modrelu_inputs(shape, special):
    z = rnd(*shape, 2, seed=11, scale=0.3)
    if special:                                                  # one element exactly 0, several below every threshold used here
        flat = z.view(-1, 2)
        flat[5] = 0.
        flat[9:14] *= 0.01
    return z


@pytest.mark.parametrize('shape,special', [((2, 4, 33, 21), False), ((1, 3, 5, 7), True)])
@pytest.mark.parametrize('b', [-0.2, 0., 0.3])
def test_modrelu_and_abs_forward_backward(ops, shape, special, b):
    z = modrelu_inputs(shape, special)
    G, Ga = rnd(*shape, 2, seed=12), rnd(*shape, seed=13)
    mod = z.double().pow(2).sum(-1).sqrt()
    away = mod > 0 if special else torch.ones_like(mod, dtype=torch.bool)
    assert float((mod[away] + b).abs().min()) > 1e-5             # the seed keeps every |z| + b away from the kink
    if special:
        assert int((mod == 0).sum()) == 1 and int((mod + b <= 0).sum()) >= (5 if b < 0 else 0)
    r64, r32 = modrelu_ref(z, b, G, F64), modrelu_ref(z, b, G, F32)
    zd, bd, Gd = z.to(dev()), torch.tensor(b, device=dev()), G.to(dev())
    y = ops.modrelu(zd, bd)
    dz, db = ops.modrelu_bwd(Gd, zd, bd)
    for name, g, a, c in zip(('modrelu y', 'modrelu dz', 'modrelu db'), (y, dz, db), r64, r32):
        if float(a.abs().max()) == 0.:
            assert float(g.abs().max()) == 0., name
        else:
            check(name, g, a, c)
    if special:                                                  # at z = 0 torch gives relu(b) + 0i and no gradient to z
        assert y.view(-1, 2)[5].tolist() == [max(float(bd), 0.), 0.] and dz.view(-1, 2)[5].tolist() == [0., 0.]
    a64, a32 = abs_ref(z, Ga, F64), abs_ref(z, Ga, F32)
    ya = ops.complex_abs(zd)
    dza = ops.complex_abs_bwd(Ga.to(dev()), zd)
    check('|z|', ya, a64[0], a32[0])
    check('d|z|', dza, a64[1], a32[1])
    dz2, db2 = ops.modrelu_bwd(Gd, zd, bd)
    assert torch.equal(y, ops.modrelu(zd, bd)) and torch.equal(dz, dz2) and torch.equal(db, db2)
    assert torch.equal(ya, ops.complex_abs(zd)) and torch.equal(dza, ops.complex_abs_bwd(Ga.to(dev()), zd))


def l1c_ref(a, b, dtype):
    a, b = (t.detach().clone().to(dtype).requires_grad_() for t in (a, b))
    out = F.l1_loss(torch.view_as_complex(a), torch.view_as_complex(b))
    (out * 1.7).backward()
    return out.detach().reshape(1), a.grad, b.grad


@pytest.mark.parametrize('shape', [(2, 1, 11), (3, 5, 4099)])
def test_complex_l1_mean(ops, shape):
    a, b = rnd(*shape, 2, seed=14), rnd(*shape, 2, seed=15)
    b.view(-1, 2)[3] = a.view(-1, 2)[3]                          # one pair of equal elements: no gradient there
    r64, r32 = l1c_ref(a, b, F64), l1c_ref(a, b, F32)
    ad, bd, g = a.to(dev()), b.to(dev()), torch.tensor(1.7, device=dev())
    out = ops.loss_mean(ops.LOSS_L1_COMPLEX, ad, bd)
    da, db = ops.loss_mean_bwd(ops.LOSS_L1_COMPLEX, ad, bd, g)
    check('mean |a - b|', out.reshape(1), r64[0], r32[0])
    check('da', da, r64[1], r32[1])
    check('db', db, r64[2], r32[2])
    assert da.view(-1, 2)[3].tolist() == [0., 0.] and db.view(-1, 2)[3].tolist() == [0., 0.]
    da2, db2 = ops.loss_mean_bwd(ops.LOSS_L1_COMPLEX, ad, bd, g)
    assert torch.equal(out, ops.loss_mean(ops.LOSS_L1_COMPLEX, ad, bd)) and torch.equal(da, da2) and torch.equal(db, db2)
    from audiolm_pytorch_amd import discriminators as D
    ac, bc = torch.view_as_complex(ad).requires_grad_(), torch.view_as_complex(bd)
    loss = D.l1_loss(ac, bc)
    (loss * 1.7).backward()
    assert torch.equal(loss.detach(), out) and torch.equal(torch.view_as_real(ac.grad), da)


# ---------------------------------------------------------------------------------------------- the module

def module_pair(ctor, logits_abs, seed, b_scale=0.1):
    import audiolm_pytorch_amd as A
    torch.manual_seed(seed)
    ours = A.ComplexSTFTDiscriminator(**ctor, logits_abs=logits_abs)
    sd = {k: v.clone() for k, v in ours.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith('.b'):                                     # ModReLU's b is initialised to 0: give every one its own non-zero value
            sd[k] = torch.randn((), generator=g) * b_scale
    ours.load_state_dict(sd)
    ref = ComplexSTFTDiscriminatorRestated(**ctor, logits_abs=logits_abs)
    ref.load_state_dict(sd, strict=True)
    return ours.to(dev()), ref


def module_ref(ref, wave, cots, dtype):
    ref = ref.to(dtype)
    ref.zero_grad(set_to_none=True)
    x = wave.detach().clone().to(dtype).requires_grad_()
    ref.probe(True)
    logits, inter = ref(x, return_intermediates=True)
    pre = ref.pre_activations().double()
    ref.probe(False)
    loss = (logits * cots[0].to(dtype)).sum() + sum((torch.view_as_real(t) * c.to(dtype)).sum() for t, c in zip(inter, cots[1:]))
    loss.backward()
    grads = {k: p.grad.clone() for k, p in ref.named_parameters()}
    return logits.detach(), [torch.view_as_real(t.detach()) for t in inter], x.grad, grads, pre


@pytest.mark.parametrize('logits_abs', [True, False])
@pytest.mark.parametrize('name,ctor,n,seed,b_scale', [('default', {}, 2560, 22, 0.03), ('small', SMALL, 320, 21, 0.1)])
def test_module_matches_the_float64_restatement(name, ctor, n, seed, b_scale, logits_abs):
    """(seed, spread of the ModReLU b): chosen so that the margin asserted below holds -- at the default size a million pre-activations pass
    through the ModReLUs; with b spread over 0.1 and seed 21 two of them fell within ten fp32 errors of the kink (the nearest 3.5e-8 from zero), and
    that one flipped element moved every upstream gradient by about 1e-4"""
    ours, ref = module_pair(ctor, logits_abs, seed, b_scale)
    wave = rnd(2, 1, n, seed=22, scale=0.3)
    with torch.no_grad():
        shapes = [tuple(t.shape) for t in (lambda o: [o[0], *(torch.view_as_real(t) for t in o[1])])(ref(wave, return_intermediates=True))]
    cots = [rnd(*s, seed=30 + i) for i, s in enumerate(shapes)]
    r64 = module_ref(ref, wave, cots, F64)
    r32 = module_ref(ref, wave, cots, F32)
    # the seed keeps every ModReLU |z| + b further from zero than ten times its own fp32 deviation: no fp32 evaluation lands across the kink
    unsafe = int((r64[4].abs() <= 10. * (r32[4] - r64[4]).abs()).sum())
    print(f'{name}: {r64[4].numel()} ModReLU pre-activations, the nearest {float(r64[4].abs().min()):.3e} from zero, {unsafe} within ten fp32 errors')
    assert unsafe == 0
    x = wave.to(dev()).requires_grad_()
    logits, inter = ours(x, return_intermediates=True)
    assert all(t.dtype == torch.complex64 for t in inter) and len(inter) == len(ours.layers) + 1
    assert logits.dtype == F32 and tuple(logits.shape) == shapes[0]
    loss = (logits * cots[0].to(dev())).sum() + sum((torch.view_as_real(t) * c.to(dev())).sum() for t, c in zip(inter, cots[1:]))
    loss.backward()
    check(f'{name} logits', logits.detach(), r64[0], r32[0])
    for i, t in enumerate(inter):
        check(f'{name} intermediate {i}', torch.view_as_real(t.detach()), r64[1][i], r32[1][i])
    check(f'{name} d wave', x.grad, r64[2], r32[2])
    for k, p in ours.named_parameters():
        check(f'{name} d {k}', p.grad, r64[3][k], r32[3][k])
    with torch.no_grad():
        assert torch.equal(ours(x), logits.detach())             # the forward-only path issues the same launches


def test_the_autograd_rule(monkeypatch):
    from audiolm_pytorch_amd import ops as _ops
    ours, _ = module_pair(SMALL, True, seed=23)
    calls = []
    real_bwd = _ops.stft_bwd
    monkeypatch.setattr(_ops, 'stft_bwd', lambda *a, **k: calls.append(1) or real_bwd(*a, **k))
    wave = rnd(2, 1, 320, seed=24, scale=0.3).to(dev())
    with torch.no_grad():
        logits, inter = ours(wave.clone().requires_grad_(), return_intermediates=True)
    assert logits.grad_fn is None and not logits.requires_grad and all(t.grad_fn is None for t in inter)
    ours.requires_grad_(False)
    logits = ours(wave)
    assert logits.grad_fn is None and not logits.requires_grad   # frozen parameters, a wave without grad: forward launches only
    x = wave.clone().requires_grad_()
    ours(x).sum().backward()                                     # frozen parameters, the wave requires grad: the generator's situation
    assert x.grad is not None and len(calls) == 1 and all(p.grad is None for p in ours.parameters())
    ours.requires_grad_(True)
    ours(wave).sum().backward()                                  # the discriminator's situation: no input gradient, no STFT backward launch
    assert len(calls) == 1 and all(p.grad is not None for p in ours.parameters())


def test_module_refusals():
    import audiolm_pytorch_amd as A
    ours = A.ComplexSTFTDiscriminator(**SMALL).to(dev())
    with pytest.raises(TypeError, match='fp32'):
        ours(torch.zeros(1, 1, 320, device=dev(), dtype=torch.float64))
    with pytest.raises(ValueError, match='too short'):
        ours(torch.zeros(1, 1, 32, device=dev()))


# ---------------------------------------------------------------------------------------------- SoundStream's loss branches

@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_losses_stft.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def _soundstream(golden, stft=True):
    import audiolm_pytorch_amd as A
    fx, sd = golden
    ss = A.SoundStream(**fx['ctor'], stft_discriminator=stft, with_discriminators=True)
    ss.load_state_dict(sd, strict=True)
    ss.to(dev()).train()
    ss.rq.eval()                                                 # deterministic quantiser, like the maker
    return ss


def _key_tol(fx, key):
    return max(TOL, 10. * fx['fp32_deviation'][key])


def _digest_check(fx, tag, grads, digests):
    worst = 0.
    for k, d in digests.items():
        if d is None:
            assert grads[k] is None, k
            continue
        assert grads[k] is not None, k
        tol = _key_tol(fx, f'{tag}:{k}')
        flat = grads[k].detach().float().reshape(-1).cpu()
        if d['norm'] == 0.:
            assert float(flat.abs().max()) <= tol, (tag, k)
            continue
        e = max(relmax(flat[::d['stride']], d['sample']), abs(float(flat.double().norm()) - d['norm']) / d['norm'])
        worst = max(worst, e)
        if k.startswith('stft_discriminator.') or e > 0.5 * tol:
            print(f'{tag} {k}: digest deviation {e:.3e} (bound {tol:.3e})')
        assert e <= tol, (tag, k, e, tol)
    print(f'{tag}: worst gradient digest deviation {worst:.3e} over {len(digests)} tensors')


def _losses_and_grads(ss, wave):
    names = [k for k, _ in ss.named_parameters() if k.startswith(('decoder.', 'discriminators.', 'stft_discriminator.'))]
    params = dict(ss.named_parameters())
    ss.zero_grad(set_to_none=True)
    total, breakdown = ss(wave, return_loss_breakdown=True)
    total.backward()
    gen = {k: (None if params[k].grad is None else params[k].grad.clone()) for k in names}
    ss.zero_grad(set_to_none=True)
    discr = ss(wave, return_discr_loss=True)
    discr.backward()
    dis = {k: (None if params[k].grad is None else params[k].grad.clone()) for k in names}
    with torch.no_grad():
        sep = ss(wave, return_discr_loss=True, return_discr_losses_separately=True)
    return total.detach(), [b.detach() for b in breakdown], gen, discr.detach(), dis, sep


def test_loss_branches_match_the_reference(golden):
    fx, _ = golden
    ss = _soundstream(golden)
    assert {k: tuple(v.shape) for k, v in ss.state_dict().items() if k.startswith('stft_discriminator.')} == fx['stft_discriminator_shapes']
    wave = fx['inputs']['wave'].to(dev())
    want = fx['outputs']['losses']
    total, breakdown, gen, discr, dis, sep = _losses_and_grads(ss, wave)

    def check_loss(key, got, ref):
        e, tol = relmax(got.reshape(1), ref.reshape(1)), _key_tol(fx, key)
        print(f'{key}: {float(got):.9g} against {float(ref):.9g}: rel {e:.3e} (bound {tol:.3e})')
        assert e <= tol, (key, e, tol)

    for name, got in zip(('recon', 'multi_spectral', 'adversarial', 'feature', 'commitment'), breakdown):
        if float(want[name]) == 0.:
            assert float(got) == 0., name
        else:
            check_loss(f'loss:{name}', got, want[name])
    check_loss('loss:total', total, want['total'])
    _digest_check(fx, 'gen', gen, fx['outputs']['gen_grads'])
    check_loss('loss:discr', discr, want['discr'])
    _digest_check(fx, 'discr', dis, fx['outputs']['discr_grads'])
    assert [n for n, _ in sep] == [n for n, _ in fx['outputs']['separately']] == ['scale:1', 'scale:0.5', 'scale:0.25', 'stft']
    for (n, got), (_, ref) in zip(sep, fx['outputs']['separately']):
        check_loss(f'separately:{n}', got, ref)

    # determinism: the same two steps again, every gradient bitwise the first's
    total2, _, gen2, discr2, dis2, _ = _losses_and_grads(ss, wave)
    assert torch.equal(total2, total) and torch.equal(discr2, discr)
    for a, b in ((gen, gen2), (dis, dis2)):
        differ = [k for k in a if (a[k] is None) != (b[k] is None) or (a[k] is not None and not torch.equal(a[k], b[k]))]
        assert not differ, differ

    # an instance handed in takes the same path as stft_discriminator=True
    import audiolm_pytorch_amd as A
    handed = _soundstream(golden, A.ComplexSTFTDiscriminator())
    total3, _, gen3, discr3, dis3, _ = _losses_and_grads(handed, wave)
    assert torch.equal(total3, total) and torch.equal(discr3, discr)
    for a, b in ((gen, gen3), (dis, dis3)):
        differ = [k for k in a if (a[k] is None) != (b[k] is None) or (a[k] is not None and not torch.equal(a[k], b[k]))]
        assert not differ, differ


def test_sgd_steps_follow_the_float64_restatement(golden):
    """three plain SGD steps in place, generator / discriminator / generator: every loss follows the float64 restatement, so each launch reads the
    parameters' current values (the complex conv kernels take the parameter's own storage)"""
    fx, sd = golden
    ss = _soundstream(golden)
    strides = (2, 4, 5, 8)
    wave = fx['inputs']['wave']
    xd = wave.to(dev())
    with torch.no_grad():
        quantized = ss(xd, return_encoded=True)[0]               # the eval-mode quantiser passes no gradient on: fixed for the whole test
    q64 = quantized.double().cpu().transpose(1, 2)
    real64 = wave.double()[:, None, :]
    discrs = [R.MultiScaleDiscriminatorRestated().double() for _ in range(3)]
    for i, d in enumerate(discrs):
        d.load_state_dict({k[len(f'discriminators.{i}.'):]: v.double() for k, v in sd.items() if k.startswith(f'discriminators.{i}.')}, strict=True)
    stft = ComplexSTFTDiscriminatorRestated()
    stft.load_state_dict({k[len('stft_discriminator.'):]: v for k, v in sd.items() if k.startswith('stft_discriminator.')}, strict=True)
    stft.double()
    dec = {k: v.double().clone().requires_grad_() for k, v in sd.items() if k.startswith('decoder.')}
    factors = (None, 2, 2)
    d_params = [*(p for d in discrs for p in d.parameters()), *stft.parameters()]
    lr_d, lr_g = 2e-3, 2e-4

    def ref_losses():
        fake = O.soundstream_decoder(dec, q64, strides=strides)
        d_loss = R.discr_loss(discrs, factors, stft, real64, fake.detach())[0]
        recon, adv, feat = R.generator_losses(discrs, factors, stft, real64, fake)
        return d_loss, recon * ss.recon_loss_weight + adv * ss.adversarial_loss_weight + feat * ss.feature_loss_weight

    def ref_step(which):
        for p in [*dec.values(), *d_params]:
            p.grad = None
        d_loss, g_loss = ref_losses()
        (d_loss if which == 'd' else g_loss).backward()
        with torch.no_grad():
            for p in (d_params if which == 'd' else list(dec.values())):
                p.add_(p.grad, alpha=-(lr_d if which == 'd' else lr_g))
        return float(d_loss.detach()), float(g_loss.detach())

    def gpu_step(which):
        ss.zero_grad(set_to_none=True)
        with torch.no_grad():
            other = ss(xd) if which == 'd' else ss(xd, return_discr_loss=True)
        loss = ss(xd, return_discr_loss=True) if which == 'd' else ss(xd)
        loss.backward()
        with torch.no_grad():
            for p in ([*ss.discriminators.parameters(), *ss.stft_discriminator.parameters()] if which == 'd' else ss.non_discr_parameters()):
                if p.grad is not None:
                    p.add_(p.grad, alpha=-(lr_d if which == 'd' else lr_g))
        loss = loss.detach()
        return (float(loss), float(other)) if which == 'd' else (float(other), float(loss))

    got, want = [], []
    for which in 'gdg':
        want.append(ref_step(which))
        got.append(gpu_step(which))
    with torch.no_grad():
        want.append(tuple(float(v) for v in ref_losses()))
        got.append((float(ss(xd, return_discr_loss=True)), float(ss(xd))))
    print('losses (discriminator, generator) per step:', got, 'float64:', want)
    tol = max(_key_tol(fx, 'loss:total'), _key_tol(fx, 'loss:discr'))
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert abs(a - b) <= tol * abs(b), (got, want)
