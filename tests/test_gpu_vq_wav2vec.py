"""GPU: audiolm_pytorch_amd.FairseqVQWav2Vec (csrc/vq_wav2vec.hip through the C ABI) against the restated vq-wav2vec (tests/vq_wav2vec_restated.py) in
fp64 on the host.

Every bound is computed in fp64 from the same operands; none is taken from what the kernels return.

GroupNorm kernels: a first-order bound in the manner of test_gpu_hubert._gn_case.  With S u the relative error of one partial's fp32 sums, dc the
rounding of one element (0 where the input is given), sigma^2 the biased variance of the block and cmax = max |x|:
    e    = dc + S u sigma + 2 u cmax                  a partial's mean (its sum, its storage as a float) and the final float mean
    dvar = (S + 8) u var + 4 sigma e + 2 e^2          the centred sums of squares, the elements and the partial means they are merged from
    rr   = dvar / (2 (var + eps)) + 2 u               relative error of rstd
    |dy| <= 1.2 |gamma| ((dc + e) rstd + |z| rr) + 16 u (|want| + 1)
Summation structure assumed.  alm_vqw2v_group_stats: a chunk of 4096 elements is summed as 16 terms per thread, 6 shuffle levels, 2 levels over the
waves (S = 24, + 2 for d = x - m0 and its square), centred on the chunk's own mean, the chunks merged in fp64.  alm_vqw2v_conv0_stats: the per-
(channel, chunk) partials of the HuBERT kernel, two levels of 32 terms (S = 64), merged in fp64.  ReLU and log(|x| + 1) are 1-Lipschitz, the skip
connection scales the bound by sqrt(residual_scale).

The whole-model rules are the ones the feature was specified with.  Features: max over (frame, group) of |ze_native - ze_fp64| / |ze_fp64| at most
8 x the same statistic of the restatement run in fp32 on the CPU.  Ids: equal on every *decided* (frame, group): the fp64 gap between the two nearest
codes > 2 e_f + 6 sqrt(K) u sum (|x| + |c|)^2 / (2 d) (test_gpu_hubert.decided_mask with K = var_dim), e_f the largest error the feature rule
permits; undecided entries may be at most 2 %.

Measured on an MI355X (this file, -s): see DESIGN.md section 'FairseqVQWav2Vec'.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import vq_wav2vec_restated as VR
from common import GOLDEN_DIR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F64 = torch.float64
EPS = 1e-5
GS_CHUNK = 4096                                                       # csrc/vq_wav2vec.hip
TINY_CONV = [(40, 10, 5), (40, 4, 2), (40, 1, 1)]


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
    assert got.shape == want.shape
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (what, ratio)


def gn_bounds(c, G, gamma, S, dc=0.0):
    """c fp64 [B, C, T] -> (z, mean, rstd, mean bound, rstd relative bound, |dy| bound without the 16 u term), module docstring; statistics per
    (sample, group) broadcast back to [B, C, T]"""
    B, C, T = c.shape
    blk = c.reshape(B, G, -1)
    mean, var = blk.mean(-1, keepdim=True), blk.var(-1, unbiased=False, keepdim=True)
    sigma, cmax = var.sqrt(), blk.abs().amax(-1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    e = dc + S * U * sigma + 2 * U * cmax
    rr = ((S + 8) * U * var + 4 * sigma * e + 2 * e * e) / (2 * (var + EPS)) + 2 * U
    z = ((blk - mean) * rstd).reshape(B, C, T)
    full = lambda t: t.expand(B, G, C // G * T).reshape(B, C, T)
    dy = 1.2 * gamma.double().abs()[None, :, None] * (full((dc + e) * rstd) + z.abs() * full(rr))
    return z, mean, rstd, e, rr, dy


def hard_rows(x):
    """[4, ...] rows: plain, a +1e3 DC offset (E[x^2] - E[x]^2 in fp32 would cancel completely), a constant block (variance 0 -> beta), a step at
    mid-length (the chunk means differ, the merge has to carry it)"""
    x = x.clone()
    x[1] += 1e3
    x[2] = 0.5
    x[3, ..., x.shape[-1] // 2:] += 50.
    return x


# ---------------------------------------------------------------- group statistics and the apply variants
GN_SHAPES = [(1, 512, 1), (1, 512, 3199), (2, 512, 98), (1, 40, 70), (2, 40, 33),
             (2, 2, GS_CHUNK), (2, 2, GS_CHUNK + 1), (2, 2, 2 * GS_CHUNK + 3)]       # a group of exactly one chunk, one chunk + 1, two chunks + 3


@pytest.mark.parametrize('G, C, T', GN_SHAPES)
def test_group_statistics_and_every_apply_variant(G, C, T):
    ops = OPS()
    x = hard_rows(rnd(4, C, T, seed=C + T))
    gamma, beta = 1 + rnd(C, seed=2, scale=0.1), rnd(C, seed=3, scale=0.1)
    z, mean, rstd, e, rr, dy = gn_bounds(x.double(), G, gamma, S=26)
    plain = z * gamma.double()[None, :, None] + beta.double()[None, :, None]
    assert float((plain - F.group_norm(x.double(), G, gamma.double(), beta.double(), EPS)).abs().max()) <= 1e-9
    xd, gd, bd = x.to(dev()), gamma.to(dev()), beta.to(dev())

    stats = ops.vqw2v_group_stats(xd, G)
    assert stats.shape == (4, G, 2) and torch.equal(stats, ops.vqw2v_group_stats(xd, G))
    s = stats.cpu().double()
    m_ratio = float(((s[..., 0:1] - mean).abs() / (e + 1e-30)).max())
    r_ratio = float(((s[..., 1:2] - rstd).abs() / (rr * rstd)).max())
    print(f'G{G} C{C} T{T}: mean err / bound {m_ratio:.3f}, rstd err / bound {r_ratio:.3f}')
    assert m_ratio <= 1.0 and r_ratio <= 1.0
    assert float((s[2, :, 1] - EPS ** -0.5).abs().max()) <= 1e-3 * EPS ** -0.5       # the constant block: variance 0, and the output is beta

    tol = lambda want, lip=1.0: lip * dy + 16 * U * (want.abs() + 1)
    run = lambda **kw: ops.vqw2v_group_apply(xd.clone(), stats, gd, bd, **kw)
    check(run(), plain, tol(plain), 'plain')
    check(run(relu=True), F.relu(plain), tol(plain), 'relu')
    want = (F.relu(plain).abs() + 1).log()
    check(run(relu=True, log_compression=True), want, tol(plain), 'relu + log')
    scale = math.sqrt(0.5)
    for rstep in (1, 2):                                         # the residual at time stride r_T // T, a sample longer than rstep T (as an odd r_T is)
        res = rnd(4, C, rstep * T + (rstep - 1 if T > 1 else 0), seed=7 + rstep)
        assert res.shape[2] // T == rstep
        want = (F.relu(plain) + res.double()[..., ::rstep][..., :T]) * scale
        got = run(relu=True, residual=res.to(dev()), residual_scale=scale)
        check(got, want, tol(want, scale) + 4 * U * res.double()[..., ::rstep][..., :T].abs(), f'relu + skip stride {rstep}')
        check(run(relu=True, residual=res.to(dev()), residual_scale=scale, log_compression=True), (want.abs() + 1).log(),
              tol(want, scale) + 4 * U * res.double()[..., ::rstep][..., :T].abs(), f'relu + skip stride {rstep} + log')
        assert torch.equal(got, run(relu=True, residual=res.to(dev()), residual_scale=scale))
    yt = ops.vqw2v_group_apply_t(xd, stats, gd, bd)
    check(yt, plain.transpose(1, 2), tol(plain).transpose(1, 2), 'transposed store')
    assert yt.is_contiguous() and torch.equal(yt, ops.vqw2v_group_apply_t(xd, stats, gd, bd))
    assert torch.equal(run(), yt.transpose(1, 2))                # the two stores hold the same numbers
    assert torch.equal(xd.cpu(), x)                              # only the in-place call writes its input


def test_group_kernels_refuse_bad_shapes():
    from audiolm_pytorch_amd import _lib
    ops = OPS()
    with pytest.raises(_lib.AlmError):
        ops.vqw2v_group_stats(torch.zeros(1, 40, 8, device=dev()), 3)        # 3 groups do not divide 40 channels
    x, st, g = torch.zeros(1, 4, 8, device=dev()), torch.zeros(1, 1, 2, device=dev()), torch.ones(4, device=dev())
    with pytest.raises(AssertionError):
        ops.vqw2v_group_apply(x, st, g, g, residual=torch.zeros(1, 4, 7, device=dev()))      # a residual shorter than the output


# ---------------------------------------------------------------- layer 0 fused: conv + GroupNorm(1, C) + ReLU, the raw activation never stored
@pytest.mark.parametrize('T', [10, 14, 16405])
def test_layer0_fused(T):
    ops = OPS()
    w = rnd(512, 10, seed=1, scale=0.3)
    gamma, beta = 1 + rnd(512, seed=2, scale=0.1), rnd(512, seed=3, scale=0.1)
    wave = hard_rows(rnd(4, T, seed=T, scale=0.3))
    c = F.conv1d(wave.double()[:, None], w.double()[:, None], stride=5)
    want = F.relu(F.group_norm(c, 1, gamma.double(), beta.double(), EPS))
    # dc = rounding of one conv output (10 fma, as test_gpu_hubert._gn_case), the largest of the sample
    dc = (10 + 2) * U * F.conv1d(wave.double().abs()[:, None], w.double().abs()[:, None], stride=5).amax((1, 2), keepdim=True)
    z, mean, rstd, e, rr, dy = gn_bounds(c, 1, gamma, S=64, dc=dc)
    wd, gd, bd = wave.to(dev()), gamma.to(dev()), beta.to(dev())
    stats = ops.vqw2v_conv0_stats(wd, w.to(dev()), 5)
    y = ops.vqw2v_conv0_apply(wd, w.to(dev()), stats, gd, bd, 5)
    assert stats.shape == (4, 1, 2) and y.shape == (4, 512, (T - 10) // 5 + 1)
    s = stats.cpu().double()
    m_ratio, r_ratio = float(((s[..., 0:1] - mean).abs() / e).max()), float(((s[..., 1:2] - rstd).abs() / (rr * rstd)).max())
    print(f'layer 0 T{T}: mean err / bound {m_ratio:.3f}, rstd err / bound {r_ratio:.3f}')
    assert m_ratio <= 1.0 and r_ratio <= 1.0
    check(y, want, dy + 16 * U * (want.abs() + 1), f'layer 0 T{T}')
    ylog = ops.vqw2v_conv0_apply(wd, w.to(dev()), stats, gd, bd, 5, log_compression=True)
    check(ylog, (want + 1).log(), dy + 16 * U * (want.abs() + 1), f'layer 0 T{T} + log')
    assert torch.equal(stats, ops.vqw2v_conv0_stats(wd, w.to(dev()), 5))
    assert torch.equal(y, ops.vqw2v_conv0_apply(wd, w.to(dev()), stats, gd, bd, 5))
    # the unfused route computes the same function: conv, statistics of the stored activation, apply
    c32 = ops.conv1d_valid(wd[:, None].contiguous(), w[:, None].contiguous().to(dev()), stride=5)
    y2 = ops.vqw2v_group_apply(c32, ops.vqw2v_group_stats(c32, 1), gd, bd, relu=True)
    check(y2, want, dy + 16 * U * (want.abs() + 1), f'layer 0 T{T} unfused')


# ---------------------------------------------------------------- assignment
def decided_mask(f64, E, e_f, never=None):
    """[B, n, G] bool: fp64 gap between the two nearest codes of the group > 2 e_f + the fp32 rounding of the two distances (module docstring);
    test_gpu_hubert.decided_mask per group.  `never`: a code that cannot win (the later copy of an exact duplicate)"""
    d = VR.distances(f64, E)
    if never is not None:
        d[..., never] = float('inf')
    two, idx = d.topk(2, dim=-1, largest=False)
    xn = f64.norm(dim=-1, keepdim=True)
    cn = torch.stack([VR.codes(E, g).double().norm(dim=-1)[idx[:, :, g]] for g in range(f64.shape[2])], dim=2)
    K = f64.shape[-1]
    rounding = (6 * math.sqrt(K) * U * (xn + cn) ** 2 / (2 * two.clamp_min(1e-30))).sum(-1)
    return (two[..., 1] - two[..., 0]) > 2 * e_f + rounding, idx[..., 0], two


@pytest.mark.parametrize('combine', [False, True])
def test_assignment_first_index_on_ties(combine):
    conv = [(512, 10, 5)]
    sd = VR.random_state_dict(4, conv=conv, combine_groups=combine)
    E = rnd(320, 1 if combine else 2, 256, seed=11)
    E[160] = E[3]                                                 # an exact duplicate code: the first index has to win
    sd['vector_quantizer.embedding'] = E
    m = A().FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=conv).to(dev())
    assert m.combine_groups == combine and m.groups == 2 and m.codebook_size == 320
    ze = rnd(2, 150, 2, 256, seed=12)
    ze[0, 5, 0] = E[3, 0] + 0.01 * rnd(256, seed=9)             # a planted near-hit of the duplicated code, in each group
    ze[1, 7, 1] = E[3, -1] + 0.01 * rnd(256, seed=10)
    ids = m.assign(ze.to(dev()))
    assert ids.dtype == torch.long and ids.shape == (2, 150, 2) and ids.is_contiguous()
    ids = ids.cpu()
    assert int(ids[0, 5, 0]) == 3 and int(ids[1, 7, 1]) == 3
    dec, want, _ = decided_mask(ze.double(), E, torch.zeros(2, 150, 2, dtype=F64), never=160)      # the duplicate never wins
    assert bool(dec[0, 5, 0]) and bool(dec[1, 7, 1]) and int(want[0, 5, 0]) == int(want[1, 7, 1]) == 3
    assert not (want == 160).any() and torch.equal(VR.assign(ze.double(), E)[dec & (want != 3)], want[dec & (want != 3)])
    assert int(dec.sum()) >= 0.99 * dec.numel()
    assert torch.equal(ids[dec], want[dec])
    assert torch.equal(m.assign(ze.to(dev())).cpu(), ids)


# ---------------------------------------------------------------- the whole model
def draw_codebook(sd, clips, num_vars, **config):
    """codes near real features: fp64 features of other clips, `num_vars` random (frame, group-pair) rows + 0.05 randn (fairseq's 0.01 randn initial
    embedding puts every code at the origin and decides nothing)"""
    f = VR.features(sd, clips, F64, **config)
    rows = f.reshape(-1, f.shape[2], f.shape[3])
    g = torch.Generator().manual_seed(78)
    E = (rows[torch.randperm(rows.shape[0], generator=g)[:num_vars]] + 0.05 * torch.randn(num_vars, *rows.shape[1:], generator=g, dtype=F64)).float()
    return E[:, :1].contiguous() if sd['vector_quantizer.embedding'].shape[1] == 1 and rows.shape[1] > 1 else E


def model_rules(sd, m, wave, what, **config):
    E = sd['vector_quantizer.embedding']
    f64 = VR.features(sd, wave, F64, **config)
    f32 = VR.features(sd, wave, torch.float32, **config).double()
    nat = m.features(wave.to(dev()))
    assert nat.dtype == torch.float32 and nat.shape == f64.shape == (wave.shape[0], m_frames(m, wave.shape[1]), m.groups, m.dim // m.groups)
    nat = nat.cpu().double()
    norm = f64.norm(dim=-1)
    e_nat, e_cpu = (nat - f64).norm(dim=-1), (f32 - f64).norm(dim=-1)
    r_nat, r_cpu = float((e_nat / norm).max()), float((e_cpu / norm).max())
    print(f'{what}: max e_f native {float(e_nat.max()):.3e} (rel {r_nat:.3e}), fp32 CPU restatement {float(e_cpu.max()):.3e} (rel {r_cpu:.3e}), '
          f'ratio {r_nat / r_cpu:.2f} (bound 8)')
    ids = m(wave.to(dev()), flatten=False).cpu()
    dec, want, two = decided_mask(f64, E, 8 * r_cpu * norm)         # e_f: the largest error the feature rule permits
    und = int((~dec).sum())
    print(f'{what}: {und} of {dec.numel()} undecided ({100 * und / dec.numel():.2f} %), equal on {int((ids[dec] == want[dec]).sum())} of {int(dec.sum())} '
          f'decided, smallest gap {float((two[..., 1] - two[..., 0]).min()):.3e}, {ids.unique().numel()} distinct ids')
    assert r_nat <= 8 * r_cpu
    assert ids.dtype == torch.long and ids.shape == dec.shape
    assert und <= 0.02 * dec.numel()
    assert torch.equal(ids[dec], want[dec])
    return ids


def m_frames(m, T):
    from audiolm_pytorch_amd.vq_wav2vec import frame_count
    return frame_count(T, m.conv_layers)


@pytest.fixture(scope='module')
def base():
    """released size (8 conv layers of 512 channels, 2 groups of 320 codes), random weights"""
    sd = VR.random_state_dict(1)
    sd['vector_quantizer.embedding'] = draw_codebook(sd, rnd(4, 16000, seed=77, scale=0.3), 320)
    return sd, A().FairseqVQWav2Vec.from_state_dict(sd).to(dev())


def test_released_size_features_and_ids(base):
    sd, m = base
    ids = model_rules(sd, m, rnd(2, 16000, seed=5, scale=0.3), 'released 2 x 16000')
    assert ids.shape == (2, 98, 2)


def test_released_size_long_row(base):
    sd, m = base
    ids = model_rules(sd, m, rnd(1, 160000, seed=6, scale=0.3), 'released 1 x 160000')
    assert ids.shape == (1, 998, 2)


VARIANTS = {
    'skip': (dict(), dict(skip_connections=True), dict(skip_connections_feature_extractor=True)),
    'non_affine': (dict(affine=False), dict(), dict(non_affine_group_norm=True)),
    'no_log': (dict(), dict(log_compression=False), dict(log_compression=False)),
    'combine_groups': (dict(combine_groups=True), dict(), dict(combine_groups=True)),
}


@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_variants_at_a_tiny_size(name):
    """C = 40, 2 groups of 16 codes of width 20; skip connections at residual time strides 2 (layer 1) and 1 (layer 2)"""
    sd_kw, oracle_kw, config = VARIANTS[name]
    sd = VR.random_state_dict(2, conv=TINY_CONV, groups=2, num_vars=16, **sd_kw)
    sd['vector_quantizer.embedding'] = draw_codebook(sd, rnd(4, 4000, seed=77, scale=0.3), 16, conv=TINY_CONV, **oracle_kw)
    m = A().FairseqVQWav2Vec.from_state_dict(sd, conv_feature_layers=TINY_CONV, **config).to(dev())
    ids = model_rules(sd, m, rnd(2, 4000, seed=5, scale=0.3), f'tiny {name}', conv=TINY_CONV, **oracle_kw)
    assert ids.shape == (2, 398, 2)


# ---------------------------------------------------------------- plumbing
def test_resample_curtail_and_flatten(base):
    sd, m = base
    assert m.target_sample_hz == 24000
    for hz in (16000, 44100):
        wave = rnd(2, int(0.25 * hz), seed=hz, scale=0.3).to(dev())
        a, b = m(wave, input_sample_hz=hz), m(A().resample(wave, hz, 24000))
        assert torch.equal(a, b) and a.dim() == 2 and a.shape[1] > 0
    wave = rnd(2, 8000 + 123, seed=3, scale=0.3).to(dev())
    m2 = A().FairseqVQWav2Vec.from_state_dict(sd, seq_len_multiple_of=160).to(dev())
    assert torch.equal(m2(wave), m(wave[:, :8000])) and m2(wave, flatten=False).shape == (2, 48, 2)
    three, flat = m(wave, flatten=False), m(wave)
    assert flat.shape == (2, 2 * three.shape[1]) and torch.equal(flat, three.reshape(2, -1))       # time-major, the groups interleaved
    assert torch.equal(flat[:, 0::2], three[..., 0]) and torch.equal(flat[:, 1::2], three[..., 1])


def test_short_wave_and_bad_arguments(base):
    from audiolm_pytorch_amd import _lib
    sd, m = base
    with pytest.raises(_lib.AlmError, match='too short'):
        m(torch.zeros(1, 464, device=dev()))
    assert m(torch.zeros(1, 465, device=dev()), flatten=False).shape == (1, 1, 2)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 800, device=dev()))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 800))


def test_batch_rows_are_independent_and_runs_are_bitwise_identical(base):
    sd, m = base
    wave = rnd(3, 8000, seed=8, scale=0.3).to(dev())
    f3, f3b = m.features(wave), m.features(wave)
    assert torch.equal(f3, f3b) and torch.equal(m(wave), m(wave))
    for r in range(3):
        assert torch.equal(m.features(wave[r:r + 1]), f3[r:r + 1])
        assert torch.equal(m(wave[r:r + 1]), m(wave)[r:r + 1])


# ---------------------------------------------------------------- the wrappers
def _codec(nq=6):
    from common import synth_state_dict
    fx = torch.load(os.path.join(GOLDEN_DIR, 'soundstream_small.pt'), weights_only=False)
    ss = A().SoundStream(**dict(fx['ctor'], target_sample_hz=16000, rq_num_quantizers=nq))
    ss.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in ss.state_dict().items()}, fx['seed']), strict=False)
    return ss.to(dev())


def test_wrappers_take_raw_wave_with_grouped_ids():
    """forward(raw_wave=...) of both wrappers = forward(semantic_token_ids=the native grouped ids), bitwise on the loss; AudioLM constructs"""
    a = A()
    sd = VR.random_state_dict(2, conv=TINY_CONV, groups=2, num_vars=16)
    sd['vector_quantizer.embedding'] = draw_codebook(sd, rnd(4, 4000, seed=77, scale=0.3), 16, conv=TINY_CONV)
    m = a.FairseqVQWav2Vec.from_state_dict(sd, target_sample_hz=16000, conv_feature_layers=TINY_CONV).to(dev())
    ss = _codec()
    T = ss.seq_len_multiple_of * max(1, 8000 // ss.seq_len_multiple_of)
    wave = rnd(2, T, seed=21, scale=0.3).to(dev())
    ids = m(wave, flatten=False)
    assert ids.shape == (2, m_frames(m, T), 2) and ids.dtype == torch.long and ids.unique().numel() > 4
    sem = a.SemanticTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=m.codebook_size, flash_attn=True).to(dev())
    w = a.SemanticTransformerWrapper(transformer=sem, wav2vec=m, unique_consecutive=False, mask_prob=0.)
    w.eval()
    la, lb = w(raw_wave=wave, return_loss=True), w(semantic_token_ids=ids, return_loss=True)
    assert torch.isfinite(la) and float(la.detach()) == float(lb.detach())
    coarse = a.CoarseTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=m.codebook_size, codebook_size=32, num_coarse_quantizers=3,
                                 flash_attn=True).to(dev())
    cw = a.CoarseTransformerWrapper(transformer=coarse, codec=ss, wav2vec=m, unique_consecutive=False, mask_prob=0.)
    cw.eval()
    la, lb = cw(raw_wave=wave, return_loss=True), cw(semantic_token_ids=ids, raw_wave_for_codec=wave, return_loss=True)
    assert torch.isfinite(la) and float(la.detach()) == float(lb.detach())
    fine = a.FineTransformer(dim=64, depth=1, heads=2, codebook_size=32, num_coarse_quantizers=3, num_fine_quantizers=3, flash_attn=True).to(dev())
    lm = a.AudioLM(wav2vec=m, codec=ss, semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    assert lm.semantic.wav2vec is m and lm.coarse.wav2vec is m
