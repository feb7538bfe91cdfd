"""Wave discriminators of SoundStream training on the MI355X (csrc/discr.hip, audiolm_pytorch_amd/discriminators.py, the loss branches of soundstream.py).

Op level: y / dx / dW / db of the grouped strided zero-padded conv (+ LeakyReLU(0.1)) against float64 CPU autograd of F.conv1d(..., groups=) +
F.leaky_relu, the pooling against F.avg_pool1d, the loss means against float64.  Module: MultiScaleDiscriminator at its defaults against the float64
restatement of tests/discr_restated.py.  End to end: the loss branches of SoundStream.forward against the REAL reference
(tests/golden/soundstream_losses_small.pt, tests/golden/make_discr_golden.py), `stft_discriminator=False` against the hand composition of the same
pieces, SGD steps against the float64 restatement, and a SoundStream built as before.

Tolerance: rel-max <= 2e-5, the project's fp32 conv tolerance (tests/test_gpu_codec_bwd.py).  For the end-to-end fixture the bound is the larger of 2e-5
and ten times the deviation of the same computation in fp32 on the CPU from float64, which the maker measured as 2.9e-6 (stored as `fp32_deviation`):
2.9e-5; the factor ten allows for another summation order.  Seeds are chosen so that no LeakyReLU pre-activation of the float64 reference lies within
1e-5 of zero (asserted; for the end-to-end fixture see the maker's docstring: at 1,041,920 pre-activations per pass no seed can keep that margin, the
maker asserts a margin of ten measured fp32 errors instead).  Every gradient is bitwise reproducible (no atomics): two runs are torch.equal."""
import os

import pytest
import torch
import torch.nn.functional as F

import audiolm_oracle as O
import discr_restated as R
from common import GOLDEN_DIR, synth_state_dict

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
GAP = 1e-5


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def check(name, got, ref, tol=TOL):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    e = relmax(got, ref)
    print(f'{name}: rel-max {e:.3e}')
    assert e <= tol, (name, e)


@pytest.fixture(scope='module')
def ops():
    from audiolm_pytorch_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------- conv

# (B, Cin, Cout, T, k, stride, pad, groups, leaky, seed): every layer shape of the reference module, an input shorter than the kernel, both activations
CONV_CASES = [(2, 1, 16, 301, 15, 1, 7, 1, False, 1), (2, 1, 16, 301, 15, 1, 7, 1, True, 1),
              (2, 16, 64, 301, 41, 4, 20, 4, True, 2), (2, 16, 64, 301, 41, 4, 20, 4, False, 2),
              (1, 64, 256, 77, 41, 4, 20, 16, True, 3),
              (2, 1024, 1024, 9, 41, 4, 20, 256, True, 4),
              (1, 16, 64, 5, 41, 4, 20, 4, True, 5),
              (2, 1024, 1024, 3, 5, 1, 2, 1, True, 6),
              (2, 1024, 1, 3, 3, 1, 1, 1, False, 7), (2, 1024, 1, 3, 3, 1, 1, 1, True, 7)]


def conv_case(B, Cin, Cout, T, k, stride, pad, groups, leaky, seed):
    """inputs and the float64 CPU autograd reference of one case: (x, w, b, g), (y, dx, dW, db), smallest |pre-activation|"""
    x = rnd(B, Cin, T, seed=100 * seed)
    w = rnd(Cout, Cin // groups, k, seed=100 * seed + 1, scale=(Cin // groups * k) ** -0.5)
    b = rnd(Cout, seed=100 * seed + 2, scale=0.1)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    pre = F.conv1d(x64, w64, b64, stride=stride, padding=pad, groups=groups)
    y = F.leaky_relu(pre, 0.1) if leaky else pre
    g = rnd(*y.shape, seed=100 * seed + 3)
    y.backward(g.double())
    return (x, w, b, g), (y.detach(), x64.grad, w64.grad, b64.grad), float(pre.detach().abs().min())


@pytest.mark.parametrize('B,Cin,Cout,T,k,stride,pad,groups,leaky,seed', CONV_CASES)
def test_grouped_conv_forward_backward(ops, B, Cin, Cout, T, k, stride, pad, groups, leaky, seed):
    (x, w, b, g), ref, gap = conv_case(B, Cin, Cout, T, k, stride, pad, groups, leaky, seed)
    assert not leaky or gap > GAP, f'a pre-activation lies {gap:.3g} from the LeakyReLU kink: choose another seed'
    xd, wd, bd, gd = (t.to(dev()) for t in (x, w, b, g))
    kw = dict(stride=stride, padding=pad, groups=groups)
    runs = []
    for _ in range(2):
        y = ops.gconv1d(xd, wd, bd, leaky=leaky, **kw)
        ys = y if leaky else None
        dx = ops.gconv1d_dgrad(gd, ys, wd, Cin, T, **kw)
        dw, db = ops.gconv1d_wgrad(gd, ys, xd, k, **kw)
        runs.append((y, dx, dw, db))
    for name, got, want in zip(('y', 'dx', 'dW', 'db'), runs[0], ref):
        check(name, got, want)
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two runs differ'


def test_conv_autograd_function_and_graph_rule():
    """conv1d_act builds a graph only when something requires grad, skips the input gradient when the input does not need one, and refuses the CPU"""
    from audiolm_pytorch_amd import discriminators as D
    conv = torch.nn.Conv1d(8, 16, 5, stride=2, padding=2, groups=2).to(dev())
    x = rnd(2, 8, 37, seed=9).to(dev())
    y = D.conv1d_act(conv, x, leaky=True)
    assert y.grad_fn is not None
    y.sum().backward()
    assert conv.weight.grad is not None and conv.bias.grad is not None and x.grad is None
    with torch.no_grad():
        assert D.conv1d_act(conv, x, leaky=True).grad_fn is None
    conv.requires_grad_(False)
    assert D.conv1d_act(conv, x, leaky=True).grad_fn is None
    xg = x.clone().requires_grad_()
    D.conv1d_act(conv, xg).sum().backward()
    assert xg.grad is not None and conv.weight.grad is not None          # the earlier gradient stays, nothing new is required
    with pytest.raises(RuntimeError, match='MI355X only'):
        D.conv1d_act(conv, x.cpu())


# ---------------------------------------------------------------------------------------------- pooling and loss means

@pytest.mark.parametrize('f,T', [(2, 64), (2, 301), (3, 300), (3, 301), (2, 1), (5, 3)])
def test_avgpool_forward_backward(ops, f, T):
    x = rnd(3, 2, T, seed=20 + T)
    x64 = x.double().requires_grad_()
    ref = F.avg_pool1d(x64, 2 * f, stride=f, padding=f)
    g = rnd(*ref.shape, seed=21 + T)
    ref.backward(g.double())
    assert ops.avgpool1d_out_len(T, f) == ref.shape[-1]
    y = ops.avgpool1d(x.to(dev()), f)
    check('y', y, ref.detach())
    check('dx', ops.avgpool1d_bwd(g.to(dev()), T, f), x64.grad)


LOSS_SEED = {(2, 1, 11): 0, (3, 5, 4099): 1}


def _loss_ref(mode, a64, b64):
    if mode == 'hinge_discr':
        return (F.relu(1 + a64) + F.relu(1 - b64)).mean()
    if mode == 'hinge_gen':
        return -a64.mean()
    return F.l1_loss(a64, b64) if mode == 'l1' else F.mse_loss(a64, b64)


# (mode, shape, seed): one block, several blocks, and for the two kink-free means the size past which a block's span doubles (> 1024 x 4096 elements)
LOSS_CASES = [(m, sh, LOSS_SEED[sh]) for m in ('hinge_discr', 'hinge_gen', 'l1', 'mse') for sh in ((2, 1, 11), (3, 5, 4099))] + \
             [(m, (1, 1, 4200001), 0) for m in ('hinge_gen', 'mse')]


def loss_inputs(shape, seed):
    return rnd(*shape, seed=310 + seed, scale=2.0), rnd(*shape, seed=320 + seed, scale=2.0)


def loss_kink_gap(a, b):
    """(smallest distance of a hinge or L1 term from its kink, clamped fractions of the two hinge terms) in float64"""
    ta, tb, d = 1 + a.double(), 1 - b.double(), (a.double() - b.double())
    return float(torch.stack((ta.abs().min(), tb.abs().min(), d.abs().min())).min()), [float((t < 0).double().mean()) for t in (ta, tb)]


@pytest.mark.parametrize('mode,shape,seed', LOSS_CASES)
def test_loss_means(mode, shape, seed):
    from audiolm_pytorch_amd import discriminators as D
    a, b = loss_inputs(shape, seed)
    if mode in ('hinge_discr', 'l1'):                            # both clamps are hit, and no term sits at a kink
        gap, clamped = loss_kink_gap(a, b)
        assert gap > GAP, f'a term lies {gap:.3g} from its kink: choose another seed'
        assert all(0.1 <= c <= 0.9 for c in clamped), clamped
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    ref = _loss_ref(mode, a64, b64)
    ref.backward()
    runs = []
    for _ in range(2):
        ad, bd = a.to(dev()).requires_grad_(), b.to(dev()).requires_grad_()
        fn = dict(hinge_discr=D.hinge_discr_loss, l1=D.l1_loss, mse=D.mse_loss).get(mode)
        loss = D.hinge_gen_loss(ad) if mode == 'hinge_gen' else fn(ad, bd)
        assert loss.shape == () and loss.dtype == F32
        (loss * 3.0).backward()
        runs.append((loss.detach(), ad.grad, None if mode == 'hinge_gen' else bd.grad))
    check('loss', runs[0][0], ref.detach())
    check('da', runs[0][1], 3.0 * a64.grad)
    if mode != 'hinge_gen':
        check('db', runs[0][2], 3.0 * b64.grad)
    assert all(x is None or torch.equal(x, y) for x, y in zip(*runs))


# ---------------------------------------------------------------------------------------------- the module

MODULE_SEED = {1000: 2, 1283: 2}


@pytest.fixture(scope='module')
def module_ref():
    """per length: float64 restatement with spread-out parameters, its logits / intermediates / gradients, computed once"""
    out = {}
    for T, seed in MODULE_SEED.items():
        ref = R.MultiScaleDiscriminatorRestated().double()
        shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        sd = {k: (2.0 * v if k.endswith('weight') else 5.0 * v) for k, v in synth_state_dict(shapes, 50 + seed).items()}     # activations of spread ~1
        ref.load_state_dict({k: v.double() for k, v in sd.items()})
        x = rnd(2, 1, T, seed=60 + seed)
        x64 = x.double().requires_grad_()
        gap, (logits, inter) = R.min_leaky_gap(ref, lambda: ref(x64, return_intermediates=True))
        gl = rnd(*logits.shape, seed=61)
        gi = [rnd(*t.shape, seed=62 + i, scale=0.05) for i, t in enumerate(inter)]
        (logits * gl.double()).sum().add(sum((t * g.double()).sum() for t, g in zip(inter, gi))).backward()
        out[T] = dict(ref=ref, sd=sd, x=x, gl=gl, gi=gi, gap=gap, logits=logits.detach(), inter=[t.detach() for t in inter], dx=x64.grad,
                      grads={k: p.grad for k, p in ref.named_parameters()})
    return out


@pytest.mark.parametrize('T', [1000, 1283])
def test_multi_scale_discriminator_matches_float64(module_ref, T):
    import audiolm_pytorch_amd as A
    r = module_ref[T]
    assert r['gap'] > GAP, f"a pre-activation lies {r['gap']:.3g} from the LeakyReLU kink: choose another seed"
    m = A.MultiScaleDiscriminator()
    m.load_state_dict({k: v.float() for k, v in r['ref'].state_dict().items()}, strict=True)
    m.to(dev())
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        x = r['x'].to(dev()).requires_grad_()
        logits, inter = m(x, return_intermediates=True)
        (logits * r['gl'].to(dev())).sum().add(sum((t * g.to(dev())).sum() for t, g in zip(inter, r['gi']))).backward()
        runs.append(dict(x=x.grad, **{k: p.grad.clone() for k, p in m.named_parameters()}))
    assert len(inter) == 4 and torch.equal(m(x.detach()), logits.detach())
    check('logits', logits.detach(), r['logits'])
    for i, (got, want) in enumerate(zip(inter, r['inter'])):
        check(f'intermediate {i}', got.detach(), want)
    check('dx', runs[0]['x'], r['dx'])
    for k, want in r['grads'].items():
        check(k, runs[0][k], want)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


# ---------------------------------------------------------------------------------------------- SoundStream's loss branches

@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_losses_small.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def _soundstream(golden, stft):
    import audiolm_pytorch_amd as A
    fx, sd = golden
    ss = A.SoundStream(**fx['ctor'], stft_discriminator=stft, with_discriminators=True)
    keep = {k: v for k, v in sd.items() if stft is not False or not k.startswith('stft_discriminator.')}
    ss.load_state_dict(keep, strict=True)
    ss.to(dev()).train()
    ss.rq.eval()                                                 # deterministic quantiser, like the maker
    return ss


def _digest_check(name, grads, digests, tol):
    worst = 0.
    for k, d in digests.items():
        if d is None:
            assert grads[k] is None, k
            continue
        assert grads[k] is not None, k
        flat = grads[k].detach().float().reshape(-1).cpu()
        if d['norm'] == 0.:                                      # final_conv.2.bias in the discriminator step: every hinge term is active, +1/n and -1/n cancel
            assert float(flat.abs().max()) <= tol, (name, k)     # relative to the sum of the terms' magnitudes, which is 2/3 here
            continue
        e = max(relmax(flat[::d['stride']], d['sample']), abs(float(flat.double().norm()) - d['norm']) / d['norm'])
        worst = max(worst, e)
        assert e <= tol, (name, k, e)
    print(f'{name}: worst gradient digest deviation {worst:.3e} over {len(digests)} tensors (bound {tol:.3e})')


def test_loss_branches_match_the_reference(golden):
    fx, _ = golden
    tol = max(TOL, 10 * fx['fp32_deviation'])
    assert tol < 1e-4
    ss = _soundstream(golden, R.TinyWaveDiscriminator())
    assert {k: tuple(v.shape) for k, v in ss.state_dict().items() if k.startswith('discriminators.')} == fx['discriminator_shapes']
    wave = fx['inputs']['wave'].to(dev())
    want = fx['outputs']['losses']
    names = [k for k, _ in ss.named_parameters() if k.startswith(('decoder.', 'discriminators.', 'stft_discriminator.'))]
    params = dict(ss.named_parameters())

    total, breakdown = ss(wave, return_loss_breakdown=True)
    assert torch.equal(ss(wave).detach(), total.detach())
    total.backward()
    for name, got in zip(('recon', 'multi_spectral', 'adversarial', 'feature', 'commitment'), breakdown):
        if float(want[name]) == 0.:
            assert float(got) == 0., name
        else:
            check(name, got.detach().reshape(1), want[name].reshape(1), tol)
    check('total', total.detach().reshape(1), want['total'].reshape(1), tol)
    gen = {k: params[k].grad for k in names}
    _digest_check('generator step', gen, fx['outputs']['gen_grads'], tol)

    ss.zero_grad(set_to_none=True)
    discr = ss(wave, return_discr_loss=True)
    discr.backward()
    check('discr', discr.detach().reshape(1), want['discr'].reshape(1), tol)
    _digest_check('discriminator step', {k: params[k].grad for k in names}, fx['outputs']['discr_grads'], tol)
    with torch.no_grad():
        sep = ss(wave, return_discr_loss=True, return_discr_losses_separately=True)
    assert [n for n, _ in sep] == [n for n, _ in fx['outputs']['separately']] == ['scale:1', 'scale:0.5', 'scale:0.25', 'stft']
    for (n, got), (_, ref) in zip(sep, fx['outputs']['separately']):
        check(n, got.reshape(1), ref.reshape(1), tol)

    # a second generator step from the same state: the loss and the wave discriminators' gradients are bitwise the first's (the decoder's also take the
    # input gradient of the caller's module, which PyTorch computes: test_without_an_stft_discriminator... checks them without it)
    ss.zero_grad(set_to_none=True)
    total2 = ss(wave)
    total2.backward()
    assert torch.equal(total2.detach(), total.detach())
    differ = [k for k in names if k.startswith('discriminators.') and not torch.equal(params[k].grad, gen[k])]
    assert not differ, differ


def test_without_an_stft_discriminator_equals_the_hand_composition(golden):
    from audiolm_pytorch_amd import discriminators as D
    fx, _ = golden
    ss = _soundstream(golden, False)
    assert not hasattr(ss, 'stft_discriminator')
    wave = fx['inputs']['wave'].to(dev())
    target = rnd(2, 2560, seed=77, scale=0.3).to(dev())
    with torch.no_grad():
        real = wave[:, None, :]
        fake = ss(wave, return_recons_only=True)
        scaled, d_losses, adv, feats = (real, fake), [], [], []
        for discr, down in zip(ss.discriminators, ss.downsamples):
            scaled = tuple(down(t) for t in scaled)
            (rl, ri), (fl, fi) = (discr(t, return_intermediates=True) for t in scaled)
            d_losses.append(D.hinge_discr_loss(fl, rl))
            adv.append(D.hinge_gen_loss(fl))
            feats.extend(D.l1_loss(r, f) for r, f in zip(ri, fi))
        recon = D.mse_loss(target[:, None, :], fake)
        adversarial, feature = torch.stack(adv).mean(), torch.stack(feats).mean()
        want_total = recon * ss.recon_loss_weight + adversarial * ss.adversarial_loss_weight + feature * ss.feature_loss_weight
        total, (g_recon, g_ms, g_adv, g_feat, g_commit) = ss(wave, target=target, return_loss_breakdown=True)
        sep = ss(wave, return_discr_loss=True, return_discr_losses_separately=True)
        d_total = ss(wave, return_discr_loss=True)
    assert len(feats) == 12 and [n for n, _ in sep] == ['scale:1', 'scale:0.5', 'scale:0.25']
    close = dict(rtol=1e-6, atol=0.)
    torch.testing.assert_close(g_recon, recon, **close)
    torch.testing.assert_close(g_adv, adversarial, **close)
    torch.testing.assert_close(g_feat, feature, **close)
    assert float(g_ms) == 0. and float(g_commit) == 0.
    torch.testing.assert_close(total, want_total, **close)
    for (_, got), want in zip(sep, d_losses):
        torch.testing.assert_close(got, want, **close)
    torch.testing.assert_close(d_total, torch.stack(d_losses).mean(), **close)

    # every gradient of both steps is bitwise reproducible
    runs = []
    for _ in range(2):
        step = []
        for kw in (dict(target=target), dict(return_discr_loss=True)):
            ss.zero_grad(set_to_none=True)
            ss(wave, **kw).backward()
            step.append({k: p.grad.clone() for k, p in ss.named_parameters() if p.grad is not None})
        runs.append(step)
    assert any(k.startswith('decoder.') for k in runs[0][0]) and not any(k.startswith('decoder.') for k in runs[0][1])
    for a, b in zip(*runs):
        differ = [k for k in a if not torch.equal(a[k], b[k])]
        assert set(a) == set(b) and not differ, differ


def test_sgd_steps_follow_the_float64_restatement(golden):
    """two discriminator steps, then two generator steps, plain SGD in place: every loss follows the float64 restatement, so each launch reads the
    parameters' current values (the conv kernels take nn.Conv1d's own storage; the decoder's weight images are rebuilt per version)"""
    fx, sd = golden
    ss = _soundstream(golden, False)
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
    dec = {k: v.double().clone().requires_grad_() for k, v in sd.items() if k.startswith('decoder.')}
    factors = (None, 2, 2)
    lr_d, lr_g = 2e-3, 2e-4

    def ref_losses():
        fake = O.soundstream_decoder(dec, q64, strides=strides)
        d_loss = R.discr_loss(discrs, factors, None, real64, fake.detach())[0]
        recon, adv, feat = R.generator_losses(discrs, factors, None, real64, fake)
        return d_loss, recon * ss.recon_loss_weight + adv * ss.adversarial_loss_weight + feat * ss.feature_loss_weight

    def ref_step(which):
        for p in [*dec.values(), *(p for d in discrs for p in d.parameters())]:
            p.grad = None
        d_loss, g_loss = ref_losses()
        (d_loss if which == 'd' else g_loss).backward()
        with torch.no_grad():
            for p in ([p for d in discrs for p in d.parameters()] if which == 'd' else list(dec.values())):
                p.add_(p.grad, alpha=-(lr_d if which == 'd' else lr_g))
        return float(d_loss.detach()), float(g_loss.detach())

    def gpu_step(which):
        ss.zero_grad(set_to_none=True)
        with torch.no_grad():
            other = ss(xd) if which == 'd' else ss(xd, return_discr_loss=True)
        loss = ss(xd, return_discr_loss=True) if which == 'd' else ss(xd)
        loss.backward()
        with torch.no_grad():
            for p in (ss.discriminators.parameters() if which == 'd' else ss.non_discr_parameters()):
                if p.grad is not None:
                    p.add_(p.grad, alpha=-(lr_d if which == 'd' else lr_g))
        loss = loss.detach()
        return (float(loss), float(other)) if which == 'd' else (float(other), float(loss))

    got, want = [], []
    for which in 'ddgg':
        want.append(ref_step(which))
        got.append(gpu_step(which))
    with torch.no_grad():
        want.append(tuple(float(v) for v in ref_losses()))
        got.append((float(ss(xd, return_discr_loss=True)), float(ss(xd))))
    print('losses (discriminator, generator) per step:', got, 'float64:', want)
    for i in range(4):                                           # every step moves its own loss by far more than the bound below
        col = 0 if i < 2 else 1
        assert abs(want[i + 1][col] - want[i][col]) > 1e-3 * abs(want[i][col]), (i, want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert abs(a - b) <= TOL * abs(b), (got, want)


def test_a_soundstream_built_as_before_is_unchanged():
    import audiolm_pytorch_amd as A
    ss = A.SoundStream(codebook_size=32, rq_num_quantizers=2, channels=4, codebook_dim=16, use_local_attn=False).to(dev())
    assert all(k.startswith(('encoder.', 'decoder.', 'rq.')) for k in ss.state_dict())
    assert not hasattr(ss, 'discriminators') and not hasattr(ss, 'downsamples') and not hasattr(ss, 'stft_discriminator')
    x = rnd(1, 640, seed=3).to(dev())
    ss.train()
    for kw in (dict(), dict(return_discr_loss=True), dict(return_loss_breakdown=True), dict(return_recons_only=True, target=x)):
        with pytest.raises(NotImplementedError):
            ss(x, **kw)
