"""GPU: audiolm_pytorch_amd.resample (csrc/resample.hip) against the restated torchaudio recipe (tests/resample_restated.py, fp32 and fp64), against
properties that do not depend on the restatement (sines, aliasing, DC), its adjoint, 64-bit addressing, and the codec / generate integration
(soundstream.py:779-795 process_input, audiolm_pytorch.py:1643-1649 / :1941-1946)."""
import math
import os

import pytest
import torch

import audiolm_oracle as O
import resample_restated as R
from common import GOLDEN_DIR, synth_state_dict

pytestmark = pytest.mark.gpu

RATES = [8000, 16000, 22050, 24000, 32000, 44100, 48000]
PAIRS = [(a, b) for a in RATES for b in RATES if a != b]


def dev():
    return torch.device('cuda:0')


def A():
    import audiolm_pytorch_amd
    return audiolm_pytorch_amd


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize('pair', PAIRS)
def test_parity_every_pair(pair):
    a, b = pair
    x = rnd(2, int(0.4 * a), seed=a // 1000 * 100 + b // 1000)
    y = A().resample(x.to(dev()), a, b).cpu()
    r32 = R.resample(x, a, b)
    r64 = R.resample(x.double(), a, b, dtype=torch.float64)
    m = float(x.abs().max())
    assert y.shape == r32.shape == (2, R.out_len(x.shape[-1], a, b)) and y.dtype == torch.float32
    assert maxerr(y, r32) <= 2e-6 * m, maxerr(y, r32)
    assert maxerr(y, r64) <= 5e-5 * m, maxerr(y, r64)


@pytest.mark.parametrize('pair,kw', [((44100, 24000), dict(resampling_method='sinc_interp_kaiser')),
                                     ((16000, 24000), dict(resampling_method='sinc_interp_kaiser', beta=8.0)),
                                     ((48000, 22050), dict(lowpass_filter_width=3, rolloff=0.9)),
                                     ((8000, 44100), dict(lowpass_filter_width=10, rolloff=0.95, resampling_method='sinc_interp_kaiser'))])
def test_parity_window_options(pair, kw):
    a, b = pair
    x = rnd(3, 5000, seed=7)
    y = A().resample(x.to(dev()), a, b, **kw).cpu()
    r = R.resample(x, a, b, lw=kw.get('lowpass_filter_width', 6), rolloff=kw.get('rolloff', 0.99),
                   method=kw.get('resampling_method', 'sinc_interp_hann'), beta=kw.get('beta'))
    assert y.shape == r.shape and maxerr(y, r) <= 2e-6 * float(x.abs().max())


def test_leading_shapes_strides_and_dtypes():
    a, b = 44100, 24000
    x = rnd(2, 3, 4001, seed=3)
    m = float(x.abs().max())
    ref = R.resample(x, a, b)
    xd = x.to(dev())
    assert maxerr(A().resample(xd, a, b).cpu(), ref) <= 2e-6 * m                      # (B, C, L)
    assert maxerr(A().resample(xd[0], a, b).cpu(), ref[0]) <= 2e-6 * m                # (B, L)
    assert maxerr(A().resample(xd[0, 1], a, b).cpu(), ref[0, 1]) <= 2e-6 * m          # (L,)
    big = rnd(3, 2, 9000, seed=4).to(dev())                                           # non-contiguous: a row-strided view and a transposed one
    v = big[:, 1, 100:4101]
    assert maxerr(A().resample(v, a, b).cpu(), R.resample(v.cpu(), a, b)) <= 2e-6 * float(v.abs().max())
    t = rnd(4001, 2, seed=5).to(dev()).t()
    assert maxerr(A().resample(t, a, b).cpu(), R.resample(t.cpu(), a, b)) <= 2e-6 * float(t.abs().max())
    xb = xd.to(torch.bfloat16)                                                        # bf16 in, fp32 arithmetic, bf16 out
    yb = A().resample(xb, a, b)
    assert yb.dtype == torch.bfloat16
    rb = R.resample(xb.float().cpu(), a, b)
    assert torch.equal(yb.cpu(), rb.to(torch.bfloat16)) or maxerr(yb.cpu(), rb) <= 2 ** -8 * float(rb.abs().max())


@pytest.mark.parametrize('pair', [(16000, 24000), (44100, 24000), (48000, 16000), (22050, 32000), (8000, 48000)])
def test_sine_matches_the_analytic_sine(pair):
    a, b = pair
    f = 0.1 * min(a, b)
    L = int(0.4 * a)
    x = torch.sin(2 * math.pi * f * torch.arange(L, dtype=torch.float64) / a).float()
    y = A().resample(x.to(dev()), a, b).cpu().double()
    want = torch.sin(2 * math.pi * f * torch.arange(y.shape[-1], dtype=torch.float64) / b)
    e = y.shape[-1] // 100
    assert maxerr(y[e:-e], want[e:-e]) <= 1.5e-3, maxerr(y[e:-e], want[e:-e])


@pytest.mark.parametrize('pair', [(48000, 16000), (44100, 24000), (44100, 16000), (48000, 24000)])
def test_tone_above_the_new_nyquist_is_suppressed(pair):
    a, b = pair
    f = 0.75 * b
    assert f < a / 2
    L = int(0.4 * a)
    x = torch.sin(2 * math.pi * f * torch.arange(L, dtype=torch.float64) / a).float()
    y = A().resample(x.to(dev()), a, b).cpu().double()
    e = y.shape[-1] // 100
    assert float(y[e:-e].pow(2).mean().sqrt()) <= 5e-3


@pytest.mark.parametrize('pair', [(16000, 24000), (44100, 24000), (24000, 8000)])
def test_constant_stays_constant(pair):
    a, b = pair
    y = A().resample(torch.ones(2, 8000, device=dev()), a, b).cpu()
    e = y.shape[-1] // 100
    assert float((y[:, e:-e] - 1).abs().max()) <= 1e-3


@pytest.mark.parametrize('pair', [(16000, 24000), (48000, 24000), (44100, 24000), (22050, 32000), (32000, 22050), (8000, 44100)])
def test_adjoint(pair):
    a, b = pair
    x = rnd(2, 3001, seed=11)
    xc = x.clone().requires_grad_(True)
    yr = R.resample(xc, a, b)
    dy = rnd(*yr.shape, seed=12)
    dx_ref, = torch.autograd.grad(yr, xc, dy)
    xd = x.to(dev()).requires_grad_(True)
    y = A().resample(xd, a, b)
    y.backward(dy.to(dev()))
    dx = xd.grad.cpu()
    assert maxerr(dx, dx_ref) <= 1e-5 * float(dx_ref.abs().max()), maxerr(dx, dx_ref)
    lhs = float((y.detach().cpu().double() * dy.double()).sum())                     # <resample(x), dy> = <x, adjoint(dy)>
    rhs = float((x.double() * dx.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), float(y.detach().abs().sum())), (lhs, rhs)
    xd2 = x.to(dev()).requires_grad_(True)                                            # bitwise deterministic (no atomics)
    y2 = A().resample(xd2, a, b)
    y2.backward(dy.to(dev()))
    assert torch.equal(y2.detach(), y.detach()) and torch.equal(xd2.grad, xd.grad)


def _check_window(y, x, a, b, s, M, row=0):
    """the recipe on x[row, s : s + M] (s a multiple of o) reproduces y[row] on every frame whose taps stay inside the slice"""
    o, n, W, T = R.geometry(a, b)
    assert s % o == 0
    L = x.shape[-1]
    M = min(M, L - s)
    ys = R.resample(x[row, s:s + M].cpu()[None], a, b)[0]
    j0 = -(-W // o)
    j1 = (M - T + W) // o + 1 if s + M < L else ys.shape[-1] // n          # at the row's end both see the same zero padding
    assert j1 > j0
    lo, hi = j0 * n, min(j1 * n, ys.shape[-1])
    full = y[row, s // o * n + lo:s // o * n + hi].cpu()
    assert maxerr(full, ys[lo:hi]) <= 2e-6 * float(x[row, s:s + M].abs().max()), (s, maxerr(full, ys[lo:hi]))


def test_thirty_second_clips_and_tile_seams():
    a, b = 44100, 24000
    x = rnd(8, 30 * a, seed=21).to(dev())
    y = A().resample(x, a, b)
    torch.cuda.synchronize()
    assert y.shape == (8, 30 * b)
    o = 147
    for row, s in [(0, 0), (3, o * 4000), (5, o * 6111), (7, (30 * a // o - 300) * o)]:
        _check_window(y, x, a, b, s, 60000, row)
    x2 = rnd(2, 30 * a, seed=22)                                                   # two full rows against the full CPU recipe, forward and adjoint
    xc = x2.clone().requires_grad_(True)
    yr = R.resample(xc, a, b)
    dy = rnd(*yr.shape, seed=23)
    dx_ref, = torch.autograd.grad(yr, xc, dy)
    xd = x2.to(dev()).requires_grad_(True)
    yd = A().resample(xd, a, b)
    yd.backward(dy.to(dev()))
    assert maxerr(yd.detach().cpu(), yr.detach()) <= 2e-6 * float(x2.abs().max())
    assert maxerr(xd.grad.cpu(), dx_ref) <= 1e-5 * float(dx_ref.abs().max())


def test_more_than_2_31_elements():
    free, _ = torch.cuda.mem_get_info()
    L = (1 << 31) + 4097
    if free < 6 * L * 4:
        pytest.skip(f'{free / 2 ** 30:.1f} GiB free on the device: the > 2^31-element input needs {6 * L * 4 / 2 ** 30:.0f} GiB')
    a, b = 48000, 24000
    g = torch.Generator(device=dev()).manual_seed(31)
    x = torch.randn(1, L, device=dev(), generator=g)
    y = A().resample(x, a, b)
    torch.cuda.synchronize()
    assert y.shape == (1, (L + 1) // 2)
    for s in [0, 2 * 700_000_000, (1 << 31) - 20000, L - 30001 - (L - 30001) % 2]:
        _check_window(y, x, a, b, s, 40000)
    del x, y
    torch.cuda.empty_cache()


def _codec(target=24000, nq=4):
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_small.pt'), weights_only=False)
    c = dict(fx['ctor'], target_sample_hz=target, rq_num_quantizers=nq)
    ss = A().SoundStream(**c)
    shapes = {k: tuple(v.shape) for k, v in ss.state_dict().items()}
    sd = synth_state_dict(shapes, fx['seed'])
    ss.load_state_dict(sd, strict=False)
    return ss.to(dev()), sd, c


def test_codec_input_sample_hz():
    ss, sd, c = _codec()
    w16 = rnd(2, 16000 // 2, seed=41) * 0.3
    wd = w16.to(dev())
    q1, i1, l1 = ss(wd, return_encoded=True, input_sample_hz=16000)
    q2, i2, l2 = ss(A().resample(wd, 16000, 24000), return_encoded=True)
    assert torch.equal(q1, q2) and torch.equal(i1, i2) and torch.equal(l1, l2)
    assert torch.equal(ss(wd, return_codes_only=True, input_sample_hz=16000), ss(A().resample(wd, 16000, 24000), return_codes_only=True))
    rec = ss(wd, return_recons_only=True, input_sample_hz=16000)
    assert rec.shape == (2, 1, (12000 // 320) * 320)
    assert torch.equal(ss(wd, return_encoded=True, input_sample_hz=24000)[1], ss(wd, return_encoded=True)[1])    # same rate: untouched
    # the codes against the oracle tokenizer on the recipe-resampled wave (float ties allowed, as in test_gpu_codec)
    wr = R.resample(w16, 16000, 24000)
    ref = O.soundstream_tokenize(sd, wr, strides=c['strides'], num_quantizers=c['rq_num_quantizers'])
    ours = i1.cpu()
    bad = (ours != ref).any(dim=-1)
    assert int(bad.sum()) <= max(1, int(1e-2 * bad.numel())), int(bad.sum())
    if bad.any():
        mult = math.prod(c['strides'])
        n = wr.shape[-1] // mult * mult
        feats = O.soundstream_encoder(sd, wr[:, :n].unsqueeze(1), strides=c['strides']).transpose(1, 2)
        cbs = [sd[f'rq.rvqs.0.layers.{q}._codebook.embed'][0] for q in range(c['rq_num_quantizers'])]
        for bi, t in torch.nonzero(bad).tolist():
            r = feats[bi, t].clone()
            for q, E in enumerate(cbs):
                d = ((r[None] - E) ** 2).sum(-1).sqrt()
                u, v = int(ours[bi, t, q]), int(ref[bi, t, q])
                if u != v:
                    assert abs(float(d[u]) - float(d[v])) <= 1e-4 * max(1.0, float(d[v])), (bi, t, q)
                    break
                r = r - E[u]


def test_generate_with_a_prime_wave_at_another_rate():
    ss, _, _ = _codec(nq=6)
    w16 = (rnd(2, 16000 // 2, seed=51) * 0.3).to(dev())
    _, idx, _ = ss(A().resample(w16, 16000, 24000), return_encoded=True)           # (b, n, 6)
    b = idx.shape[0]
    coarse = A().CoarseTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=20, codebook_size=32, num_coarse_quantizers=3, flash_attn=True).to(dev())
    cw = A().CoarseTransformerWrapper(transformer=coarse, codec=ss, unique_consecutive=False)
    sem = torch.randint(0, 20, (b, 6), generator=torch.Generator().manual_seed(52)).to(dev())
    torch.manual_seed(5)
    got = cw.generate(semantic_token_ids=sem, prime_wave=w16, prime_wave_input_sample_hz=16000, max_time_steps=4)
    torch.manual_seed(5)
    want = cw.generate(semantic_token_ids=sem, prime_coarse_token_ids=idx[..., :3].reshape(b, -1), max_time_steps=4)
    assert torch.equal(got, want)
    fine = A().FineTransformer(dim=64, depth=1, heads=2, codebook_size=32, num_coarse_quantizers=3, num_fine_quantizers=3, flash_attn=True).to(dev())
    fw = A().FineTransformerWrapper(transformer=fine, codec=ss)
    ct = idx[..., :3]
    torch.manual_seed(6)
    got = fw.generate(coarse_token_ids=ct, prime_wave=w16, prime_wave_input_sample_hz=16000)
    torch.manual_seed(6)
    want = fw.generate(coarse_token_ids=ct, prime_fine_token_ids=idx[..., 3:].reshape(b, -1))
    assert torch.equal(got, want)
