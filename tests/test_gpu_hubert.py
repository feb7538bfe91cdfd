"""GPU: audiolm_pytorch_amd.HubertWithKmeans (csrc/hubert.hip through the C ABI) against the restated HuBERT (tests/hubert_restated.py) in fp64 on the host.

Per-kernel bounds are first-order rounding bounds of a length-K fp32 dot product, |err| <= (K + c) u sum |a_i b_i| with u = 2^-24, evaluated in fp64 from
the same operands (c covers the epilogue); none is taken from what the kernels return.  The whole-model bound is the one the feature was specified
with: max over frames of the per-frame L2 error, relative to the feature norm, at most 8 x the same statistic of the restatement run in fp32 on the CPU.
Ids must be equal on every *decided* frame: fp64 gap between the nearest and second-nearest centre > 2 e_f + the fp32 rounding of the two distances.
The rounding term is 6 standard errors of a K-term fp32 sum with independent roundings, 6 sqrt(K) u (|x|^2 + |c|^2 + 2 |x| |c|) / (2 d) per distance
(the kernel forms d^2 = |x|^2 + |c|^2 - 2 x.c); undecided frames may be at most 1 % of all frames.

Measured on an MI355X (this file, -s): see DESIGN.md section 'HubertWithKmeans'.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import hubert_restated as HR
from common import GOLDEN_DIR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F64 = torch.float64


def dev():
    return torch.device('cuda:0')


def A():
    import audiolm_pytorch_amd
    return audiolm_pytorch_amd


def OPS():
    from audiolm_pytorch_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def check(got, want, tol, what):
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / tol).max())
    print(f'{what}: max abs err {float(err.max()):.3e}, max err / bound {ratio:.3f}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (what, ratio)


# ---------------------------------------------------------------- conv1d_valid: the six strided layers, ragged lengths
@pytest.mark.parametrize('k, s, Tin', [(3, 2, 799), (3, 2, 130), (3, 2, 67), (3, 2, 3), (2, 2, 200), (2, 2, 131), (2, 2, 2)])
def test_strided_conv_gelu(k, s, Tin):
    x, w = rnd(2, 512, Tin, seed=Tin), rnd(512, 512, k, seed=k, scale=(512 * k) ** -0.5)
    y = OPS().conv1d_valid(x.to(dev()), w.to(dev()), stride=s, gelu=True)
    pre = F.conv1d(x.double(), w.double(), stride=s)
    bound = (512 * k + 8) * U * F.conv1d(x.double().abs(), w.double().abs(), stride=s)
    assert y.shape == pre.shape == (2, 512, (Tin - k) // s + 1)
    check(y, F.gelu(pre), 1.2 * bound + 16 * U * (pre.abs() + 1), f'conv k{k} s{s} T{Tin}')


def test_conv_generic_kernel_size_and_small_channels():
    """a kernel size without a specialised instance (5), channel counts ragged against the 64 x 64 tile, stride 3, bias"""
    x, w, b = rnd(3, 40, 101, seed=1), rnd(70, 40, 5, seed=2, scale=0.1), rnd(70, seed=3)
    y = OPS().conv1d_valid(x.to(dev()), w.to(dev()), b.to(dev()), stride=3)
    pre = F.conv1d(x.double(), w.double(), b.double(), stride=3)
    bound = (200 + 8) * U * (F.conv1d(x.double().abs(), w.double().abs(), stride=3) + b.abs()[None, :, None])
    check(y, pre, bound + 16 * U * (pre.abs() + 1), 'conv k5 s3')


# ---------------------------------------------------------------- layer 0 + GroupNorm over time + GELU
def _gn_case(wave, w, gamma, beta, what):
    ops = OPS()
    wd, gd, bd = w.to(dev()), gamma.to(dev()), beta.to(dev())
    stats = ops.hubert_conv0_stats(wave.to(dev()), wd, 5)
    y = ops.hubert_conv0_apply(wave.to(dev()), wd, stats, gd, bd, 5)
    c = F.conv1d(wave.double()[:, None], w.double()[:, None], stride=5)
    want = F.gelu(F.group_norm(c, 512, gamma.double(), beta.double(), 1e-5))
    # dc = rounding of one conv output; it moves c, the mean (<= dc) and rstd (relative <= 2 dc / sigma, times |c - mean| / sigma <= ~4 sigmas)
    dc = (10 + 2) * U * F.conv1d(wave.double().abs()[:, None], w.double().abs()[:, None], stride=5).amax(-1, keepdim=True)
    sigma = (c.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    z = (c - c.mean(-1, keepdim=True)).abs() / sigma
    # the statistics are fp32 sums of 32 + 32 terms per level (then fp64): mean off by <= 64 u sigma, rstd by <= 32 u relative (times z)
    tol = 1.2 * gamma.double().abs()[None, :, None] * ((2 + 2 * z) * dc / sigma + 64 * U * (1 + z)) + 64 * U * (want.abs() + 1)
    assert y.shape == want.shape
    check(y, want, tol, what)
    mean = stats[..., 0].cpu().double()
    assert float(((mean - c.mean(-1)).abs() / (dc[..., 0] + 64 * U * sigma[..., 0] + 4 * U * c.mean(-1).abs() + 1e-30)).max()) <= 1.0
    return y


def test_groupnorm_gelu_plain_dc_offset_and_constant_channel():
    w = rnd(512, 10, seed=1, scale=0.3)
    w[7] = 0.                                                     # a channel whose conv output is constant (zero): variance 0 -> beta
    gamma, beta = 1 + rnd(512, seed=2, scale=0.1), rnd(512, seed=3, scale=0.1)
    wave = rnd(4, 16405, seed=4, scale=0.3)
    wave[1] += 1e3                                                # DC-heavy: E[c^2] - E[c]^2 in fp32 would cancel completely
    wave[2] = 0.5                                                 # a constant row: every channel has zero variance
    wave[3, :8000] += 50.                                         # a step: the chunk means differ, the merge has to carry it
    y = _gn_case(wave, w, gamma, beta, 'conv0 + groupnorm + gelu')
    assert float((y[:, 7].cpu().double() - F.gelu(beta[7].double())).abs().max()) <= 4 * U


def test_groupnorm_short_and_chunk_edges():
    w, gamma, beta = rnd(512, 10, seed=5, scale=0.3), torch.ones(512), torch.zeros(512)
    for T in (10, 14, 10 + 5 * 1023, 10 + 5 * 1024, 10 + 5 * 2047 + 3):      # 1 output, 1, exactly one chunk, one chunk + 1, two chunks
        _gn_case(rnd(2, T, seed=T, scale=0.5), w, gamma, beta, f'conv0 gn T{T}')


def test_groupnorm_is_deterministic():
    ops = OPS()
    w, wave = rnd(512, 10, seed=1, scale=0.3).to(dev()), rnd(3, 48000, seed=2).to(dev())
    a, b = ops.hubert_conv0_stats(wave, w, 5), ops.hubert_conv0_stats(wave, w, 5)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- positional conv
@pytest.mark.parametrize('n', [1, 63, 99, 130])
def test_positional_conv_gelu_residual(n):
    x, w, b = rnd(2, 768, n, seed=n), rnd(768, 48, 128, seed=1, scale=(48 * 128) ** -0.5), rnd(768, seed=2, scale=0.1)
    y = OPS().conv1d_valid(x.to(dev()), w.to(dev()), b.to(dev()), pad=64, groups=16, gelu=True, residual=x.to(dev()), drop_last=1)
    pre = F.conv1d(x.double(), w.double(), b.double(), padding=64, groups=16)[..., :-1]
    bound = (48 * 128 + 8) * U * (F.conv1d(x.double().abs(), w.double().abs(), padding=64, groups=16)[..., :-1] + b.abs()[None, :, None])
    assert y.shape == x.shape
    check(y, x.double() + F.gelu(pre), 1.2 * bound + 16 * U * (pre.abs() + x.double().abs() + 1), f'pos conv n{n}')


# ---------------------------------------------------------------- LayerNorm over channels
@pytest.mark.parametrize('C, n', [(512, 99), (768, 1), (768, 33), (768, 1499), (40, 70)])
def test_layernorm_over_channels(C, n):
    x, g, b = rnd(2, C, n, seed=n) * 2 + 3, 1 + rnd(C, seed=1, scale=0.1), rnd(C, seed=2, scale=0.1)
    y = OPS().layernorm_bct_split(x.to(dev()), g.to(dev()), b.to(dev()))
    want = F.layer_norm(x.double().transpose(1, 2), (C,), g.double(), b.double(), 1e-5).transpose(1, 2)
    # sums of C / 32 terms per slice + 32 slices: mean and variance carry <= (C / 32 + 32) u relative to sum |x| / C resp. the variance
    z = ((x.double() - x.double().mean(1, keepdim=True)).abs() / x.double().std(1, unbiased=False, keepdim=True).clamp_min(1e-3))
    su = (C / 32 + 40) * U
    tol = g.double().abs()[None, :, None] * (su * x.double().abs().mean(1, keepdim=True) / x.double().std(1, unbiased=False, keepdim=True).clamp_min(1e-3)
                                            + su * z + 8 * U * (z + 1)) + 8 * U * (want.abs() + 1)
    check(y, want, tol, f'layernorm C{C} n{n}')
    assert torch.equal(y, OPS().layernorm_bct_split(x.to(dev()), g.to(dev()), b.to(dev())))


# ---------------------------------------------------------------- attention
@pytest.mark.parametrize('n', [1, 63, 64, 65, 499, 1499])
def test_bidirectional_attention(n):
    B, H = (1, 12) if n > 500 else (2, 12)
    qkv = rnd(B, 3 * H * 64, n, seed=n)
    qkv[:, :2 * H * 64] *= 1.5                                    # scores with a spread of a few units: a peaked softmax, not a flat one
    y = OPS().mha_attn(qkv.to(dev()), H)
    q, k, v = (t.transpose(1, 2).double() for t in qkv.split(H * 64, dim=1))
    want = HR.attention(q, k, v, H).transpose(1, 2)
    # score rounding ds = (64 + 3) u sum |q k| <= 67 u |q| |k|; softmax weights move by <= 2 ds relatively; the P V sum over n keys adds (n + 64) u
    qn = (q.view(B, n, H, 64).norm(dim=-1) * 0.125).amax(1)       # [B, H]
    kn = k.view(B, n, H, 64).norm(dim=-1).amax(1)
    vmax = v.view(B, n, H, 64).abs().amax((1, 3))
    ds = 67 * U * qn * kn
    tol = ((4 * ds + (n + 64) * U) * vmax)[:, :, None, None].expand(B, H, 64, n).reshape(B, H * 64, n) + 16 * U
    assert y.shape == want.shape
    check(y, want, tol, f'attention n{n}')


def test_attention_rejects_other_head_widths():
    from audiolm_pytorch_amd import _lib
    with pytest.raises(_lib.AlmError):
        OPS().mha_attn(torch.zeros(1, 3 * 2 * 32, 8, device=dev()), 2, dim_head=32)


# ---------------------------------------------------------------- Linear + bias (+ GELU) (+ residual)
def test_gelu_gemm_and_residual_gemm():
    x, w1, b1 = rnd(2, 768, 99, seed=1), rnd(3072, 768, 1, seed=2, scale=768 ** -0.5), rnd(3072, seed=3, scale=0.1)
    h = OPS().conv1d_valid(x.to(dev()), w1.to(dev()), b1.to(dev()), gelu=True)
    pre = F.conv1d(x.double(), w1.double(), b1.double())
    bound = (768 + 8) * U * (F.conv1d(x.double().abs(), w1.double().abs()) + b1.abs()[None, :, None])
    check(h, F.gelu(pre), 1.2 * bound + 16 * U * (pre.abs() + 1), 'fc1 + gelu')
    hh, w2, b2 = F.gelu(pre).float(), rnd(768, 3072, 1, seed=4, scale=3072 ** -0.5), rnd(768, seed=5, scale=0.1)
    y = OPS().conv1d_valid(hh.to(dev()), w2.to(dev()), b2.to(dev()), residual=x.to(dev()))
    pre2 = F.conv1d(hh.double(), w2.double(), b2.double())
    bound2 = (3072 + 8) * U * (F.conv1d(hh.double().abs(), w2.double().abs()) + b2.abs()[None, :, None])
    check(y, x.double() + pre2, bound2 + 16 * U * (pre2.abs() + x.double().abs() + 1), 'fc2 + residual')


# ---------------------------------------------------------------- assignment
def decided_mask(f64, centres, e_f):
    """[B, n] bool: fp64 gap between the two nearest centres > 2 e_f + the fp32 rounding of the two distances (module docstring)"""
    d = HR.distances(f64, centres)
    two, idx = d.topk(2, dim=-1, largest=False)
    xn = f64.norm(dim=-1, keepdim=True)
    cn = centres.double().norm(dim=-1)[idx]
    K = f64.shape[-1]
    rounding = (6 * math.sqrt(K) * U * (xn + cn) ** 2 / (2 * two.clamp_min(1e-30))).sum(-1)
    return (two[..., 1] - two[..., 0]) > 2 * e_f + rounding, idx[..., 0], two


@pytest.mark.parametrize('C', [500, 1024])
def test_kmeans_assignment(C):
    ops = OPS()
    x, cen = rnd(1, 300, 768, seed=C), rnd(C, 768, seed=C + 1)
    cen[C // 2] = cen[3]                                          # an exact duplicate: the first index has to win
    x[0, 5] = cen[3] + 0.01 * rnd(768, seed=9)
    E = cen[None].to(dev())
    ids = ops.rvq_encode(x[0].to(dev()), E, *ops.rvq_pack(E)).view(1, 300).cpu()
    d = HR.distances(x.double(), cen)
    d[..., C // 2] = float('inf')                                 # the duplicate never wins
    dec, want, _ = decided_mask(x.double(), cen, torch.zeros(1, 300, dtype=F64))
    assert ids.dtype == torch.long and int(ids[0, 5]) == 3
    assert int(dec.sum()) >= 0.99 * 300
    assert torch.equal(ids[dec], d.argmin(-1)[dec])


# ---------------------------------------------------------------- the whole model at base size
@pytest.fixture(scope='module')
def base():
    sd = HR.random_state_dict(1, layers=9)
    clips = rnd(4, 48000, seed=77, scale=0.3)                    # 4 x 3 s of other clips: 596 frames to draw centres from
    f = HR.features(sd, clips, 9, dtype=F64).reshape(-1, 768)
    g = torch.Generator().manual_seed(78)
    centres = (f[torch.randperm(f.shape[0], generator=g)[:500]] + 0.05 * torch.randn(500, 768, generator=g, dtype=F64)).float()
    m = A().HubertWithKmeans.from_state_dict(sd, centres).to(dev())
    return sd, centres, m


def model_rules(sd, centres, m, wave, what):
    f64 = HR.features(sd, wave, 9, dtype=F64)
    f32 = HR.features(sd, wave, 9, dtype=torch.float32).double()
    nat = m.features(wave.to(dev())).cpu().double()
    assert nat.shape == f64.shape == (wave.shape[0], (wave.shape[1] - 400) // 320 + 1, 768)
    norm = f64.norm(dim=-1)
    e_nat, e_cpu = (nat - f64).norm(dim=-1), (f32 - f64).norm(dim=-1)
    r_nat, r_cpu = float((e_nat / norm).max()), float((e_cpu / norm).max())
    print(f'{what}: max_f e_f native {float(e_nat.max()):.3e} (rel {r_nat:.3e}), fp32 CPU restatement {float(e_cpu.max()):.3e} (rel {r_cpu:.3e}), '
          f'ratio {r_nat / r_cpu:.2f} (bound 8)')
    ids = m(wave.to(dev())).cpu()
    dec, want, two = decided_mask(f64, centres, e_nat)
    und = int((~dec).sum())
    print(f'{what}: {int(dec.sum())} of {dec.numel()} frames decided, equal on {int((ids[dec] == want[dec]).sum())}, smallest gap '
          f'{float((two[..., 1] - two[..., 0]).min()):.3e}, {ids.unique().numel()} distinct ids')
    assert r_nat <= 8 * r_cpu
    assert ids.dtype == torch.long and ids.shape == dec.shape
    assert und <= 0.01 * dec.numel()
    assert torch.equal(ids[dec], want[dec])
    return ids


def test_base_model_features_and_ids(base):
    sd, centres, m = base
    model_rules(sd, centres, m, rnd(2, 32000, seed=5, scale=0.3), 'base 2 x 2 s')


def test_base_model_30s_row(base):
    sd, centres, m = base
    ids = model_rules(sd, centres, m, rnd(1, 480000, seed=6, scale=0.3), 'base 1 x 30 s')
    assert ids.shape == (1, 1499)


def test_resample_then_16k_is_bitwise_and_seq_len_multiple(base):
    sd, centres, m = base
    for hz in (24000, 44100):
        wave = rnd(2, int(0.5 * hz), seed=hz, scale=0.3).to(dev())
        a = m(wave, input_sample_hz=hz)
        b = m(A().resample(wave, hz, 16000))
        assert torch.equal(a, b) and a.shape[1] == (b.shape[1])
    wave = rnd(2, 8000 + 123, seed=3, scale=0.3).to(dev())
    m2 = A().HubertWithKmeans.from_state_dict(sd, centres, seq_len_multiple_of=320).to(dev())
    assert torch.equal(m2(wave), m(wave[:, :8000])) and m2(wave).shape == (2, 24)
    assert torch.equal(m2(wave, flatten=False), m2(wave, flatten=True))


def test_batch_rows_are_independent_and_runs_are_bitwise_identical(base):
    sd, centres, m = base
    wave = rnd(3, 16000, seed=8, scale=0.3).to(dev())
    f3, f3b = m.features(wave), m.features(wave)
    assert torch.equal(f3, f3b) and torch.equal(m(wave), m(wave))
    for r in range(3):
        assert torch.equal(m.features(wave[r:r + 1]), f3[r:r + 1])
        assert torch.equal(m(wave[r:r + 1]), m(wave)[r:r + 1])


# ---------------------------------------------------------------- the recorded reference forward, the wrappers
def tiny_module(**kw):
    t = torch.load(os.path.join(GOLDEN_DIR, 'hubert_tiny.pt'), weights_only=True)
    c = t['config']
    m = A().HubertWithKmeans.from_state_dict(t['state_dict'], t['centres'], output_layer=c['layers'], conv_feature_layers=c['conv'],
                                             encoder_attention_heads=c['heads'], conv_pos_groups=c['groups'], **kw)
    return m.to(dev()), t


def test_recorded_reference_forward_reproduces():
    rec = torch.load(os.path.join(GOLDEN_DIR, 'hubert_ref_forward.pt'), weights_only=True)
    for case in rec['cases']:
        m, t = tiny_module(seq_len_multiple_of=case['seq_len_multiple_of'])
        c = t['config']
        ids = m(rec['wave'].to(dev()), flatten=case['flatten']).cpu()
        assert ids.shape == case['ids'].shape and ids.dtype == torch.long
        wave = rec['wave'] if case['seq_len_multiple_of'] is None else rec['wave'][:, :rec['wave'].shape[1] // 320 * 320]
        f64 = HR.features(t['state_dict'], wave, c['layers'], c['heads'], c['conv'], c['groups'], F64)
        nat = m.features(wave.to(dev())).cpu().double()
        dec, want, _ = decided_mask(f64, t['centres'], (nat - f64).norm(dim=-1))
        assert torch.equal(want, case['ids'])
        assert int((~dec).sum()) <= 0.01 * dec.numel()
        assert torch.equal(ids[dec], case['ids'][dec])


def _codec(nq=6):
    from common import synth_state_dict
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_small.pt'), weights_only=False)
    ss = A().SoundStream(**dict(fx['ctor'], target_sample_hz=16000, rq_num_quantizers=nq))
    ss.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in ss.state_dict().items()}, fx['seed']), strict=False)
    return ss.to(dev())


def test_wrappers_take_raw_wave():
    """forward(raw_wave=...) of both wrappers = forward(semantic_token_ids=native ids); generate(prime_wave=...) runs; AudioLM constructs"""
    a = A()
    m, t = tiny_module()
    ss = _codec()
    T = ss.seq_len_multiple_of * max(1, 8000 // ss.seq_len_multiple_of)
    wave = rnd(2, T, seed=21, scale=0.3).to(dev())
    ids = m(wave, flatten=False)
    assert ids.shape == (2, (T - 400) // 320 + 1) and ids.dtype == torch.long
    sem = a.SemanticTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=m.codebook_size, flash_attn=True).to(dev())
    w = a.SemanticTransformerWrapper(transformer=sem, wav2vec=m, unique_consecutive=False, mask_prob=0.)
    w.eval()
    la, lb = w(raw_wave=wave, return_loss=True), w(semantic_token_ids=ids, return_loss=True)
    assert torch.isfinite(la) and float(la.detach()) == float(lb.detach())
    prime = rnd(1, 6000, seed=22, scale=0.3).to(dev())
    out = w.generate(prime_wave=prime, prime_wave_input_sample_hz=24000, max_length=20)
    assert out.dtype == torch.long and out.shape[0] == 1 and out.shape[1] >= 1

    coarse = a.CoarseTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=m.codebook_size, codebook_size=32, num_coarse_quantizers=3,
                                 flash_attn=True).to(dev())
    cw = a.CoarseTransformerWrapper(transformer=coarse, codec=ss, wav2vec=m, unique_consecutive=False, mask_prob=0.)
    cw.eval()
    la, lb = cw(raw_wave=wave, return_loss=True), cw(semantic_token_ids=ids, raw_wave_for_codec=wave, return_loss=True)
    assert torch.isfinite(la) and float(la.detach()) == float(lb.detach())
    fine = a.FineTransformer(dim=64, depth=1, heads=2, codebook_size=32, num_coarse_quantizers=3, num_fine_quantizers=3, flash_attn=True).to(dev())
    lm = a.AudioLM(wav2vec=m, codec=ss, semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    assert lm.semantic.wav2vec is m and lm.coarse.wav2vec is m
