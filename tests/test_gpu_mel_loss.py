"""Multi-spectral mel-spectrogram reconstruction loss of SoundStream training on the MI355X (csrc/mel_loss.hip, audiolm_pytorch_amd/mel_loss.py, the
generator loss of soundstream.py).

Op level: `MelSpectrogram` (value, gradient under a random cotangent) and one scale of `multi_spectral_recon_loss` (value, d / d recon) against float64
torch autograd of the restatement (tests/mel_restated.py: torch.stft + matmul), at shapes where every tile dimension is ragged, the window is shorter
than n_fft (restricted reduction range), F = 257 leaves a one-row reduction tail and n_mels = 80 needs two row tiles; the rows that must contribute an
exact 0 (silence on both sides, recon == orig, an empty mel filter).  Module level: the six scales of the reference defaults on 2 x 1280 samples.  End
to end: the generator loss of SoundStream(with_mel_loss=True) against the REAL reference run over the restated MelSpectrogram
(tests/golden/soundstream_losses_mel.pt, tests/golden/make_mel_loss_golden.py).

Tolerance: the rule of tests/test_gpu_stft_discr.py -- the larger of 2e-5 rel-max and ten times the deviation of the same quantity evaluated in fp32 on
the CPU from float64 (computed here; per key from the fixture).  Every measured error is printed.  Results are bitwise reproducible (no atomics)."""
import copy
import os

import pytest
import torch

from common import GOLDEN_DIR, synth_state_dict
from mel_restated import MelSpectrogramRestated, multi_spectral_recon_loss_restated

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


def check(name, got, ref64, ref32):
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    e, floor = relmax(got, ref64), relmax(ref32, ref64)
    tol = max(TOL, 10. * floor)
    print(f'{name}: rel-max {e:.3e} (fp32 on the CPU {floor:.3e}, bound {tol:.3e})')
    assert e <= tol, (name, e, tol)


# (B, n, n_fft, win, hop, n_mels, normalized)
OP_CASES = [(3, 200, 64, 64, 16, 20, False),      # every tile dimension ragged; one empty filter
            (2, 333, 128, 32, 8, 64, False),      # window shorter than n_fft: the reduction runs over [48, 80); two column tiles
            (2, 640, 512, 64, 16, 80, False),     # F = 257 = 8 * 32 + 1; two row tiles of the mel projection
            (3, 200, 64, 64, 16, 20, True)]


def transforms(n_fft, win, hop, n_mels, normalized):
    import audiolm_pytorch_amd as A
    kw = dict(sample_rate=16000, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, normalized=normalized)
    return A.MelSpectrogram(**kw).to(dev()), MelSpectrogramRestated(**kw)


def mel_ref(ref, x, G, dtype):
    ref = copy.deepcopy(ref).to(dtype)
    x = x.detach().clone().to(dtype).requires_grad_()
    mel = ref(x)
    (mel * G.to(dtype)).sum().backward()
    return mel.detach(), x.grad


def loss_ref(refs, alphas, orig, recon, dtype):
    refs = [copy.deepcopy(r).to(dtype) for r in refs]
    x = recon.detach().clone().to(dtype).requires_grad_()
    loss = multi_spectral_recon_loss_restated(orig.to(dtype), x, refs, alphas)
    (loss * 1.7).backward()
    return loss.detach().reshape(1), x.grad


def loss_ours(ours, alphas, orig, recon):
    import audiolm_pytorch_amd as A
    x = recon.to(dev()).requires_grad_()
    loss = A.multi_spectral_recon_loss(orig.to(dev()), x, ours, alphas)
    (loss * 1.7).backward()
    return loss.detach().reshape(1), x.grad


@pytest.mark.parametrize('B,n,n_fft,win,hop,n_mels,normalized', OP_CASES)
def test_mel_spectrogram_forward_backward(B, n, n_fft, win, hop, n_mels, normalized):
    ours, ref = transforms(n_fft, win, hop, n_mels, normalized)
    x = rnd(B, n, seed=3, scale=0.5)
    T = n // hop + 1
    G = rnd(B, n_mels, T, seed=4)
    m64, dx64 = mel_ref(ref, x, G, F64)
    m32, dx32 = mel_ref(ref, x, G, F32)
    if (n_fft, n_mels) == (64, 20):
        assert int((ref.mel_scale.fb.abs().sum(0) == 0).sum()) == 1          # the case has an empty filter

    def run():
        xd = x.to(dev()).requires_grad_()
        mel = ours(xd)
        (mel * G.to(dev())).sum().backward()
        return mel.detach(), xd.grad

    mel, dx = run()
    assert tuple(mel.shape) == (B, n_mels, T)
    check('mel', mel, m64, m32)
    check('d wave', dx, dx64, dx32)
    empty = (ref.mel_scale.fb.abs().sum(0) == 0).nonzero().reshape(-1).tolist()
    assert all(float(mel[:, m].abs().max()) == 0. for m in empty)
    mel2, dx2 = run()
    assert torch.equal(mel, mel2) and torch.equal(dx, dx2)
    with torch.no_grad():
        assert torch.equal(ours(x.to(dev())), mel)               # the forward-only path issues the same launches
    assert torch.equal(ours(x.to(dev()).reshape(B, 1, n)), mel.reshape(B, 1, n_mels, T))


@pytest.mark.parametrize('B,n,n_fft,win,hop,n_mels,normalized', OP_CASES)
def test_one_scale_of_the_loss(B, n, n_fft, win, hop, n_mels, normalized):
    ours, ref = transforms(n_fft, win, hop, n_mels, normalized)
    alphas = [(win / 2) ** 0.5]
    orig, recon = rnd(B, n, seed=5, scale=0.5), rnd(B, n, seed=6, scale=0.4)
    l64, g64 = loss_ref([ref], alphas, orig, recon, F64)
    l32, g32 = loss_ref([ref], alphas, orig, recon, F32)
    loss, g = loss_ours([ours], alphas, orig, recon)
    check('loss', loss, l64, l32)
    check('d recon', g, g64, g32)
    loss2, g2 = loss_ours([ours], alphas, orig, recon)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)
    with torch.no_grad():                                        # no graph: the same value from the forward launches alone
        import audiolm_pytorch_amd as A
        assert torch.equal(A.multi_spectral_recon_loss(orig.to(dev()), recon.to(dev()), [ours], alphas).reshape(1), loss)


def test_rows_that_contribute_exactly_nothing():
    """row 1 silent in both waves (every mel 0: both clamps inactive, norm 0), row 2 recon == orig non-zero (sign(0), norm 0); the empty filter of the
    case sits in every row.  torch gives each an exact 0 and so must the kernels -- never 0 * inf."""
    B, n, n_fft, win, hop, n_mels, normalized = OP_CASES[0]
    ours, ref = transforms(n_fft, win, hop, n_mels, normalized)
    alphas = [(win / 2) ** 0.5]
    orig, recon = rnd(B, n, seed=7, scale=0.5), rnd(B, n, seed=8, scale=0.4)
    orig[1], recon[1] = 0., 0.
    recon[2] = orig[2]
    l64, g64 = loss_ref([ref], alphas, orig, recon, F64)
    l32, g32 = loss_ref([ref], alphas, orig, recon, F32)
    assert float(g64[1:].abs().max()) == 0. and float(g64[0].abs().max()) > 0.
    loss, g = loss_ours([ours], alphas, orig, recon)
    check('loss', loss, l64, l32)
    check('d recon', g, g64, g32)
    assert bool(torch.isfinite(g).all()) and float(g[1:].abs().max()) == 0.
    rest, grest = loss_ours([ours], alphas, orig[1:], recon[1:])
    assert float(rest) == 0. and bool(torch.isfinite(grest).all()) and float(grest.abs().max()) == 0.
    only, _ = loss_ours([ours], alphas, orig[:1], recon[:1])    # the mean is over all three rows: row 0 alone weighs three times as much
    assert abs(float(only) - 3. * float(loss)) <= 1e-5 * abs(float(only))


def default_scales():
    import audiolm_pytorch_amd as A
    ours, refs, alphas = [], [], []
    for p in range(6, 12):                                       # soundstream.py:650-672 at the defaults
        win = 2 ** p
        kw = dict(sample_rate=16000, n_fft=max(512, win), win_length=win, hop_length=win // 4, n_mels=64, normalized=False)
        ours.append(A.MelSpectrogram(**kw).to(dev()))
        refs.append(MelSpectrogramRestated(**kw))
        alphas.append((win / 2) ** 0.5)
    return ours, refs, alphas


def test_six_scales_at_the_reference_defaults():
    """2 x 1280 samples: the shortest multiple of 320 the 2048-point scale admits"""
    ours, refs, alphas = default_scales()
    orig, recon = rnd(2, 1, 1280, seed=9, scale=0.3), rnd(2, 1, 1280, seed=10, scale=0.25)
    for i, (t, r) in enumerate(zip(ours, refs)):
        with torch.no_grad():
            mel = t(orig.to(dev()))
            check(f'scale {i} mel', mel, r(orig.double()), copy.deepcopy(r).float()(orig))
        assert tuple(mel.shape) == (2, 1, 64, 1280 // t.hop_length + 1)
    l64, g64 = loss_ref(refs, alphas, orig, recon, F64)
    l32, g32 = loss_ref(refs, alphas, orig, recon, F32)
    loss, g = loss_ours(ours, alphas, orig, recon)
    check('six-scale loss', loss, l64, l32)
    check('six-scale d recon', g, g64, g32)
    loss2, g2 = loss_ours(ours, alphas, orig, recon)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


def test_a_loaded_window_rebuilds_the_basis():
    """the DFT basis is derived from the `window` buffer and follows it: load_state_dict of another window changes the result to that window's"""
    B, n, n_fft, win, hop, n_mels, _ = OP_CASES[1]
    ours, ref = transforms(n_fft, win, hop, n_mels, False)
    x = rnd(B, n, seed=11, scale=0.5)
    with torch.no_grad():
        before = ours(x.to(dev()))
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        sd['spectrogram.window'] = torch.hamming_window(win, dtype=F64)
        ref.load_state_dict(sd)
        ours.load_state_dict({k: v.float() for k, v in sd.items()})
        after = ours(x.to(dev()))
        check('mel under the loaded window', after, ref(x.double()), copy.deepcopy(ref).float()(x))
    assert not torch.equal(before, after)


# ---------------------------------------------------------------------------------------------- SoundStream's generator loss

@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_losses_mel.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def _soundstream(golden):
    import audiolm_pytorch_amd as A
    fx, sd = golden
    ss = A.SoundStream(**fx['ctor'], with_discriminators=True, stft_discriminator=True, with_mel_loss=True)
    missing, unexpected = ss.load_state_dict(sd, strict=False)   # the mel buffers keep their constructed values, as in the maker
    assert not unexpected and missing and all(k.startswith('mel_spec_transforms.') for k in missing)
    ss.to(dev()).train()
    ss.rq.eval()                                                 # deterministic quantiser, like the maker
    return ss


def _key_tol(fx, key):
    return max(TOL, 10. * fx['fp32_deviation'][key])


def _digest_check(fx, tag, grads, digests):
    worst = 0.
    for k, d in digests.items():
        tol = _key_tol(fx, f'{tag}:{k}')
        flat = grads[k].detach().float().reshape(-1).cpu()
        e = max(relmax(flat[::d['stride']], d['sample']), abs(float(flat.double().norm()) - d['norm']) / d['norm'])
        worst = max(worst, e)
        print(f'{tag} {k}: digest deviation {e:.3e} (bound {tol:.3e})')
        assert e <= tol, (tag, k, e, tol)
    print(f'{tag}: worst gradient digest deviation {worst:.3e} over {len(digests)} tensors')


def _passes(ss, wave):
    params = {k: p for k, p in ss.named_parameters() if k.startswith('decoder.')}
    ss.zero_grad(set_to_none=True)
    total, breakdown = ss(wave, return_loss_breakdown=True)
    total.backward()
    gen = {k: p.grad.clone() for k, p in params.items()}
    ss.zero_grad(set_to_none=True)
    _, breakdown2 = ss(wave, return_loss_breakdown=True)
    breakdown2[1].backward()                                     # the mel term alone
    mel = {k: p.grad.clone() for k, p in params.items()}
    ss.zero_grad(set_to_none=True)
    return total.detach(), [b.detach() for b in breakdown], gen, mel


def test_generator_loss_matches_the_reference(golden):
    fx, _ = golden
    ss = _soundstream(golden)
    assert {k: tuple(v.shape) for k, v in ss.state_dict().items() if k.startswith('mel_spec_transforms.')} == fx['mel_spec_transforms_shapes']
    wave = fx['inputs']['wave'].to(dev())
    want = fx['outputs']['losses']
    total, breakdown, gen, mel = _passes(ss, wave)

    def check_loss(key, got, ref):
        e, tol = relmax(got.reshape(1), ref.reshape(1)), _key_tol(fx, key)
        print(f'{key}: {float(got):.9g} against {float(ref):.9g}: rel {e:.3e} (bound {tol:.3e})')
        assert e <= tol, (key, e, tol)

    assert float(want['multi_spectral']) > 0.
    for name, got in zip(('recon', 'multi_spectral', 'adversarial', 'feature', 'commitment'), breakdown):
        if float(want[name]) == 0.:
            assert float(got) == 0., name
        else:
            check_loss(f'loss:{name}', got, want[name])
    check_loss('loss:total', total, want['total'])
    _digest_check(fx, 'gen', gen, fx['outputs']['gen_grads'])
    _digest_check(fx, 'mel', mel, fx['outputs']['mel_grads'])

    discr = ss(wave, return_discr_loss=True)                     # the discriminator branch never touches the mel transforms: it runs on this model
    assert discr.ndim == 0 and bool(torch.isfinite(discr))

    total2, breakdown2, gen2, mel2 = _passes(ss, wave)           # determinism: every value and gradient bitwise the first's
    assert torch.equal(total2, total) and all(torch.equal(a, b) for a, b in zip(breakdown, breakdown2))
    for a, b in ((gen, gen2), (mel, mel2)):
        differ = [k for k in a if not torch.equal(a[k], b[k])]
        assert not differ, differ
