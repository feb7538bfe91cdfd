"""GPU: audiolm_pytorch_amd.EncodecWrapper (csrc/encodec.hip, csrc/codec.hip through the C ABI) against the restated EnCodec (tests/encodec_restated.py) in
fp64 on the host.  Every float bound is against that fp64 oracle and none is taken from what the kernels return:

  convolutions : the first-order rounding bound of a length-K fp32 dot product, |err| <= (K + c) u sum |w_i x_i|, u = 2^-24, evaluated in fp64 from the same
                 operands (tests/test_gpu_hubert.py); c = 16 covers the bias, the ELU on the operand (a few ulp of each term) and the epilogue; a stored
                 ELU adds 16 u (|out| + 1).  Where the weight norm is folded on the device, the fp32 norm of NW terms adds NW u to the factor.
  LSTM         : max |err| of the native run <= 8 x max |err| of torch's fp32 nn.LSTM on the CPU, both against fp64 nn.LSTM (+ skip); at T = 1, where the
                 CPU error can be a single rounding, plus an absolute floor of 4 ulp of max |y|.
  whole model  : max over frames of the per-frame L2 error relative to the feature norm <= 8 x the same statistic of the restatement run in fp32 on the CPU.
  codes        : compared level by level along the fp64 path.  A frame is *decided* up to the first level at which the fp64 gap between its two nearest
                 codes is not above 2 e + the fp32 rounding of the two distances (6 sqrt(K) u (|r| + |c|)^2 / (2 d) each, as in test_gpu_hubert.py), with
                 e = the native feature error of the frame + u |r| of every residual formed so far (each fp32 subtraction rounds the new residual once).  Decided levels must equal the oracle's
                 codes; frames that do not stay decided through every level may be at most 2 % (a cap, not a tolerance).
  decode       : relative L2 error of a row <= 8 x the fp32 CPU restatement's.

Measured on an MI355X (this file, -s): see docs/LABBOOK.md.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import encodec_restated as ER
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


def ENC():
    from audiolm_pytorch_amd import encodec
    return encodec


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def check(got, want, tol, what):
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / tol).max())
    print(f'{what}: max abs err {float(err.max()):.3e}, max err / bound {ratio:.3f}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (what, ratio)


# ---------------------------------------------------------------- convolutions with a pre-activation
def ref_conv(x, w, b, stride, dil):
    """(out, sum |w| |x| + |b|) of the causal conv in fp64: reflect left pad (k - 1) dil + 1 - stride"""
    left = dil * (w.shape[-1] - 1) + 1 - stride
    xp = F.pad(x, (left, 0), mode='reflect')
    return F.conv1d(xp, w, b, stride=stride, dilation=dil), F.conv1d(xp.abs(), w.abs(), b.abs(), stride=stride, dilation=dil)


CONVS = [(1, 4, 7, 1, 1), (32, 16, 3, 1, 1), (16, 32, 1, 1, 1), (6, 10, 3, 2, 1), (32, 64, 4, 1, 2), (64, 128, 16, 1, 8)]


@pytest.mark.parametrize('T', [7, 33, 321])
@pytest.mark.parametrize('Cin, Cout, k, dil, stride', CONVS)
def test_conv_pre_elu_bias_residual(Cin, Cout, k, dil, stride, T):
    from audiolm_pytorch_amd import _lib
    ops = OPS()
    x, w, b = rnd(2, Cin, T, seed=T + Cin), rnd(Cout, Cin, k, seed=k + Cout, scale=(Cin * k) ** -0.5), rnd(Cout, seed=3, scale=0.3)
    xd, bd, wp = x.to(dev()), b.to(dev()), ops.conv1d_pack(w.to(dev()))
    if T <= dil * (k - 1) + 1 - stride:                            # a reflect pad of 8 on 7 samples does not exist (torch refuses it too): refused, not computed
        with pytest.raises(_lib.AlmError):
            ops.conv1d_causal_pre(xd, wp, bd, Cout, k, stride=stride, dilation=dil, pre_elu=True)
        return
    Tout = T // stride
    res = rnd(2, Cout, Tout, seed=5)
    for pre in (False, True):
        xin = F.elu(x.double()) if pre else x.double()
        want, mag = ref_conv(xin, w.double(), b.double(), stride, dil)
        assert want.shape == (2, Cout, Tout)
        bound = (Cin * k + 16) * U * mag
        what = f'conv {Cin}->{Cout} k{k} d{dil} s{stride} T{T} pre{int(pre)}'
        y = ops.conv1d_causal_pre(xd, wp, bd, Cout, k, stride=stride, dilation=dil, pre_elu=pre)
        assert y.shape == want.shape
        check(y, want, bound + 4 * U * want.abs(), what)
        y = ops.conv1d_causal_pre(xd, wp, bd, Cout, k, stride=stride, dilation=dil, pre_elu=pre, elu=True)
        check(y, F.elu(want), bound + 16 * U * (want.abs() + 1), what + ' elu')
        y = ops.conv1d_causal_pre(xd, wp, bd, Cout, k, stride=stride, dilation=dil, pre_elu=pre, residual=res.to(dev()))
        check(y, want + res.double(), bound + 4 * U * (want.abs() + res.double().abs()), what + ' residual')
        if not pre and stride == 1:                                # without the flag it is the SoundStream conv, bit for bit (whose k = 2 s strided convs run another kernel)
            assert torch.equal(ops.conv1d_causal_pre(xd, wp, bd, Cout, k, stride=stride, dilation=dil),
                               ops.conv1d_causal(xd, wp, bd, Cout, k, stride=stride, dilation=dil))


SMALL = dict(num_filters=4, hidden_size=16, codebook_size=32, upsampling_ratios=[8, 2], num_lstm_layers=1)


@pytest.fixture(scope='module')
def small():
    """encoder.layers.3 = conv(4 -> 8, k 4, stride 2), .6 = conv(8 -> 16, k 16, stride 8); decoder.layers.3 = convtr(16 -> 8, stride 8), .6 = convtr(8 -> 4, stride 2)"""
    sd = ER.random_state_dict(31, num_codebooks=1, **SMALL)
    return sd, A().EncodecWrapper.from_state_dict(sd, strides=(2, 8), bandwidth=7.5, **SMALL).to(dev())


@pytest.mark.parametrize('layer, Cin, stride, T', [(6, 8, 8, 323), (3, 4, 2, 9)])
def test_ragged_length_is_reflect_padded_to_the_stride(small, layer, Cin, stride, T):
    sd, m = small
    p = f'encoder.layers.{layer}'
    x = rnd(2, Cin, T, seed=T)
    y = m._conv(p, x.to(dev()), stride=stride, pre_elu=True)
    want = ER.conv(sd, p, F.elu(x.double()), stride)
    assert y.shape == want.shape == (2, 2 * Cin, -(-T // stride))
    w = ER.folded(sd, p, F64)
    k = w.shape[-1]
    xp = F.pad(F.elu(x.double()), (k - stride, -T % stride), mode='reflect')
    mag = F.conv1d(xp.abs(), w.abs(), sd[p + '.conv.bias'].double().abs(), stride=stride)
    check(y, want, (Cin * k + 16 + Cin * k) * U * mag + 4 * U * want.abs(), f'ragged conv s{stride} T{T}')


@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('layer, Cin, stride', [(3, 16, 8), (6, 8, 2)])
def test_transposed_conv_with_folded_weight_norm(small, layer, Cin, stride, n):
    sd, m = small
    p = f'decoder.layers.{layer}'
    x = rnd(3, Cin, n, seed=n + stride)
    for pre in (False, True):
        xin = F.elu(x.double()) if pre else x.double()
        y = m._convtr(p, x.to(dev()), pre)
        want = ER.convtr(sd, p, xin, stride)
        assert y.shape == want.shape == (3, Cin // 2, n * stride)
        w, b = ER.folded(sd, p, F64), sd[p + '.conv.bias'].double()
        assert w.shape == (Cin, Cin // 2, 2 * stride)             # [Cin, Cout, k]: the norm runs per INPUT channel
        mag = F.conv_transpose1d(xin.abs(), w.abs(), b.abs(), stride=stride)[..., :n * stride]
        check(y, want, (2 * Cin + 16 + Cin // 2 * 2 * stride) * U * mag + 4 * U * want.abs(), f'convtr s{stride} n{n} pre{int(pre)}')


# ---------------------------------------------------------------- LSTM
def lstm_case(H, L, B, T):
    g = torch.Generator().manual_seed(H * 1000 + L * 100 + B * 10 + T)
    ref = torch.nn.LSTM(H, H, L)
    for prm in ref.parameters():
        prm.data = (torch.rand(prm.shape, generator=g) * 2 - 1) * H ** -0.5
    x = torch.randn(B, H, T, generator=g)
    xs = x.permute(2, 0, 1)
    with torch.no_grad():
        y32 = (ref(xs)[0] + xs).permute(1, 2, 0).double()
        ref64 = torch.nn.LSTM(H, H, L).double()
        ref64.load_state_dict({k: v.double() for k, v in ref.state_dict().items()})
        y64 = (ref64(xs.double())[0] + xs.double()).permute(1, 2, 0)
    image = ENC().lstm_image({k: v.to(dev()) for k, v in ref.state_dict().items()}, L)
    return x, image, y32, y64


@pytest.mark.parametrize('L', [1, 2])
@pytest.mark.parametrize('H', [16, 40, 512])
def test_lstm_against_fp64(H, L):
    for B in (1, 3):
        for T in (1, 2, 3, 75):
            x, image, y32, y64 = lstm_case(H, L, B, T)
            y = ENC().lstm_skip(image, x.to(dev()))
            assert y.shape == (B, H, T) and y.dtype == torch.float32 and torch.isfinite(y).all()
            e_nat, e_cpu = float((y.cpu().double() - y64).abs().max()), float((y32 - y64).abs().max())
            floor = 4 * U * float(y64.abs().max()) if T == 1 else 0.
            print(f'lstm H{H} L{L} B{B} T{T}: native {e_nat:.3e}, fp32 CPU nn.LSTM {e_cpu:.3e}, ratio {e_nat / max(e_cpu, 1e-30):.2f} (bound 8)')
            assert e_nat <= 8 * e_cpu + floor, (H, L, B, T, e_nat, e_cpu)


@pytest.mark.parametrize('H, L', [(40, 2), (512, 2), (512, 1)])
def test_lstm_runs_are_bitwise_equal_and_rows_independent(H, L):
    x, image, _, _ = lstm_case(H, L, 3, 9)
    xd = x.to(dev())
    a, b = ENC().lstm_skip(image, xd), ENC().lstm_skip(image, xd)
    assert torch.equal(a, b)
    for r in range(3):
        assert torch.equal(ENC().lstm_skip(image, xd[r:r + 1].contiguous()), a[r:r + 1])
    assert OPS().lstm_launches(9, L) == 9 + L - 1


def test_lstm_batch_larger_than_one_chunk():
    """11 rows: one full chunk of 8 and a ragged one"""
    x, image, y32, y64 = lstm_case(40, 2, 11, 5)
    y = ENC().lstm_skip(image, x.to(dev()))
    e_nat, e_cpu = float((y.cpu().double() - y64).abs().max()), float((y32 - y64).abs().max())
    print(f'lstm B11: native {e_nat:.3e}, fp32 CPU {e_cpu:.3e}')
    assert e_nat <= 8 * e_cpu
    assert torch.equal(ENC().lstm_skip(image, x[9:10].contiguous().to(dev())), y[9:10])


# ---------------------------------------------------------------- the decided rule
def decided_levels(sd, f64, e_f, n_q):
    """fp64 path, level by level -> (want [.., n_q] codes, alive [.., n_q] bool: decided at this level and every one before, smallest gap)"""
    E = ER.codebooks(sd, n_q, F64)
    r, alive, want, keep, gaps = f64, torch.ones(f64.shape[:-1], dtype=torch.bool), [], [], []
    e = e_f.clone()
    K = f64.shape[-1]
    for q in range(n_q):
        d = ER.distances(r, E[q]).clamp_min(0).sqrt()
        two, idx = d.topk(2, dim=-1, largest=False)
        rn, cn = r.norm(dim=-1, keepdim=True), E[q].norm(dim=-1)[idx]
        rounding = (6 * math.sqrt(K) * U * (rn + cn) ** 2 / (2 * two.clamp_min(1e-30))).sum(-1)
        gap = two[..., 1] - two[..., 0]
        alive = alive & (gap > 2 * e + rounding)
        first = (-ER.distances(r, E[q])).max(dim=-1).indices      # what EncodecEuclideanCodebook.quantize returns
        want.append(first)
        keep.append(alive)
        gaps.append(gap)
        r = r - E[q][first]
        e = e + U * r.norm(dim=-1)                                  # the fp32 subtraction rounds every component of the new residual once
    return torch.stack(want, -1), torch.stack(keep, -1), torch.stack(gaps, -1)


def code_rules(sd, f64, e_f, codes, n_q, what, cap=0.02):
    want, alive, gaps = decided_levels(sd, f64, e_f, n_q)
    assert torch.equal(want, ER.codes(sd, f64, n_q))
    frames = alive[..., -1].numel()
    und = int((~alive[..., -1]).sum())
    print(f'{what}: {frames - und} of {frames} frames decided through {n_q} levels ({und} undecided, cap {cap * frames:.1f}), decided levels equal on '
          f'{int((codes[alive] == want[alive]).sum())} of {int(alive.sum())}, all levels equal on {int((codes == want).sum())} of {want.numel()}, '
          f'smallest gap {float(gaps.min()):.3e}')
    assert codes.dtype == torch.long and codes.shape == want.shape
    assert und <= cap * frames
    assert torch.equal(codes[alive], want[alive])


def model_rules(sd, m, wave, what, cfg={}):
    f64 = ER.encoder(sd, wave, F64, **cfg)
    f32 = ER.encoder(sd, wave, torch.float32, **cfg).double()
    nat = m.encode(wave.to(dev())).cpu().double()
    assert nat.shape == f64.shape == (wave.shape[0], -(-wave.shape[1] // m.downsample_factor), m.codebook_dim)
    norm = f64.norm(dim=-1)
    e_nat, e_cpu = (nat - f64).norm(dim=-1), (f32 - f64).norm(dim=-1)
    r_nat, r_cpu = float((e_nat / norm).max()), float((e_cpu / norm).max())
    print(f'{what}: features rel err native {r_nat:.3e}, fp32 CPU restatement {r_cpu:.3e}, ratio {r_nat / r_cpu:.2f} (bound 8)')
    assert r_nat <= 8 * r_cpu
    _, codes, none = m(wave.to(dev()))
    assert none is None and codes.shape == (*nat.shape[:2], m.num_quantizers)
    code_rules(sd, f64, e_nat, codes.cpu(), m.num_quantizers, what)
    return codes


# ---------------------------------------------------------------- the whole model at the 24 kHz geometry
@pytest.fixture(scope='module')
def full():
    sd = ER.random_state_dict(1, zero_bias=True)                 # zero biases: with the default init they dominate and the frames collapse (module docstring of the restatement)
    return sd, A().EncodecWrapper.from_state_dict(sd).to(dev())


def test_full_model_features_and_codes(full):
    sd, m = full
    codes = model_rules(sd, m, rnd(2, 24000, seed=15, scale=0.3), '24 kHz 2 x 1 s, 6 kbps')
    assert codes.shape == (2, 75, 8) and codes.dtype == torch.long


def test_full_model_24kbps(full):
    sd, _ = full
    m = A().EncodecWrapper.from_state_dict(sd, bandwidth=24.0).to(dev())
    assert m.num_quantizers == 32
    # one clip of 4 s: 2 % of the 75 frames of a 1 s clip would be a cap of one frame
    assert model_rules(sd, m, rnd(1, 96000, seed=96, scale=0.3), '24 kHz 1 x 4 s, 24 kbps').shape == (1, 300, 32)


def test_full_model_30s_row(full):
    sd, m = full
    assert model_rules(sd, m, rnd(1, 720000, seed=7, scale=0.3), '24 kHz 1 x 30 s').shape == (1, 2250, 8)


def test_full_model_ragged_and_short(full):
    sd, m = full
    assert model_rules(sd, m, rnd(1, 24123, seed=8, scale=0.3), '24 kHz ragged 24123').shape == (1, 76, 8)
    with pytest.raises(ValueError):
        m(rnd(1, 2000, seed=9).to(dev()))


def test_full_model_decode(full):
    sd, m = full
    codes = torch.randint(1024, (3, 25, 8), generator=torch.Generator().manual_seed(10))
    y64 = ER.decode(sd, codes, F64)
    y32 = ER.decode(sd, codes, torch.float32).double()
    y = m.decode_from_codebook_indices(codes.to(dev()))
    assert y.shape == y64.shape == (3, 1, 25 * 320) and y.dtype == torch.float32
    r_nat = float(((y.cpu().double() - y64).norm(dim=-1) / y64.norm(dim=-1)).max())
    r_cpu = float(((y32 - y64).norm(dim=-1) / y64.norm(dim=-1)).max())
    print(f'decode 3 x 25 frames: rel L2 native {r_nat:.3e}, fp32 CPU restatement {r_cpu:.3e}, ratio {r_nat / r_cpu:.2f} (bound 8)')
    assert r_nat <= 8 * r_cpu
    for r in range(3):
        assert torch.equal(m.decode_from_codebook_indices(codes[r:r + 1].to(dev())), y[r:r + 1])


# ---------------------------------------------------------------- API, goldens (tiny configuration)
def tiny_module(**kw):
    t = torch.load(os.path.join(GOLDEN_DIR, 'encodec_tiny.pt'), weights_only=True)
    m = A().EncodecWrapper.from_state_dict(t['state_dict'], strides=(2, 4), bandwidth=kw.pop('bandwidth', t['bandwidth']), **dict(t['config'], **kw))
    return m.to(dev()), t


def test_api_shapes_and_bitwise_identities():
    m, t = tiny_module()
    wave = rnd(2, 3, 200, seed=11, scale=0.3).to(dev())
    emb, codes, none = m(wave, return_encoded=True)
    assert none is None and codes.shape == (2, 3, 25, 4) and codes.dtype == torch.long and emb.shape == (2, 3, 25, 16) and emb.dtype == torch.float32
    emb0, codes0, _ = m(wave)
    assert emb0 is None and torch.equal(codes0, codes)
    flat = codes.reshape(6, 25, 4)
    assert torch.equal(m.get_emb_from_indices(flat), emb.reshape(6, 25, 16))
    assert torch.equal(m.decode(emb.reshape(6, 25, 16)), m.decode_from_codebook_indices(flat))
    assert m.decode_from_codebook_indices(flat).shape == (6, 1, 200)
    w441 = rnd(2, 4410, seed=12, scale=0.3).to(dev())
    a = m(w441, input_sample_hz=44100, return_encoded=True)
    b = m(A().resample(w441, 44100, 24000), return_encoded=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and a[1].shape == (2, 300, 4)
    assert torch.equal(m(w441)[1], m(w441)[1])


def test_tiny_golden_features_codes_and_decode():
    m, t = tiny_module()
    sd, cfg = t['state_dict'], t['config']
    for name, wave in t['waves'].items():
        want = t['hf'][name]
        f64 = want['features64']
        f32 = ER.encoder(sd, wave, torch.float32, **cfg).double()
        nat = m.encode(wave.to(dev())).cpu().double()
        assert nat.shape == f64.shape
        e_nat, e_cpu = (nat - f64).norm(dim=-1), (f32 - f64).norm(dim=-1)
        r_nat, r_cpu = float((e_nat / f64.norm(dim=-1)).max()), float((e_cpu / f64.norm(dim=-1)).max())
        print(f'tiny golden {name}: features rel err native {r_nat:.3e}, fp32 CPU {r_cpu:.3e}, ratio {r_nat / r_cpu:.2f} (bound 8)')
        assert r_nat <= 8 * r_cpu
        codes = m(wave.to(dev()))[1].cpu()
        assert torch.equal(ER.codes(sd, f64, 4), want['codes'])
        code_rules(sd, f64, e_nat, codes, 4, f'tiny golden {name}')
        y64 = want['decoded64']
        y32 = ER.decode(sd, want['codes'], torch.float32, **cfg).double()
        y = m.decode_from_codebook_indices(want['codes'].to(dev())).cpu().double()
        assert y.shape == y64.shape
        r_nat, r_cpu = float(((y - y64).norm(dim=-1) / y64.norm(dim=-1)).max()), float(((y32 - y64).norm(dim=-1) / y64.norm(dim=-1)).max())
        print(f'tiny golden {name}: decode rel L2 native {r_nat:.3e}, fp32 CPU {r_cpu:.3e}, ratio {r_nat / r_cpu:.2f} (bound 8)')
        assert r_nat <= 8 * r_cpu


def test_recorded_reference_forward_reproduces():
    m, t = tiny_module()
    sd, cfg = t['state_dict'], t['config']
    rec = torch.load(os.path.join(GOLDEN_DIR, 'encodec_ref_forward.pt'), weights_only=True)
    assert m.seq_len_multiple_of == rec['seq_len_multiple_of']
    for wave, want in ((rec['wave3'], rec['encoded']), (rec['wave23'], rec['lead_dims'])):
        emb, codes, none = m(wave.to(dev()), return_encoded=True)
        assert none is None and codes.shape == want['codes'].shape and codes.dtype == want['codes'].dtype == torch.long
        assert emb.shape == want['emb'].shape and emb.dtype == torch.float32
        flat = wave.reshape(-1, wave.shape[-1])
        f64 = ER.encoder(sd, flat, F64, **cfg)
        e_nat = (m.encode(flat.to(dev())).cpu().double() - f64).norm(dim=-1)
        code_rules(sd, f64, e_nat, codes.cpu().reshape(-1, *codes.shape[-2:]), 4, 'recorded reference forward')
        same = (codes.cpu() == want['codes']).all(-1)                # emb is a sum of 4 code vectors: exact up to 4 roundings where the codes agree
        assert float((emb.cpu().double() - want['emb'])[same].abs().max()) <= 4 * U * float(want['emb'].abs().max())
    assert m(rec['wave3'].to(dev()))[0] is None
    emb = m.get_emb_from_indices(rec['codes_only'].to(dev()))
    assert float((emb.cpu().double() - rec['get_emb_from_indices']).abs().max()) <= 4 * U * float(rec['get_emb_from_indices'].abs().max())
    y = m.decode_from_codebook_indices(rec['codes_only'][:1].to(dev()))
    assert y.shape == rec['decode_b1'].shape and y.dtype == torch.float32
    y32 = ER.decode(sd, rec['codes_only'][:1], torch.float32, **cfg).double()
    r_nat = float((y.cpu().double() - rec['decode_b1']).norm() / rec['decode_b1'].norm())
    r_cpu = float((y32 - rec['decode_b1']).norm() / rec['decode_b1'].norm())
    print(f'recorded reference decode b = 1: rel L2 native {r_nat:.3e}, fp32 CPU {r_cpu:.3e}')
    assert r_nat <= 8 * r_cpu


# ---------------------------------------------------------------- the wrappers take it as their codec
def test_wrappers_take_the_codec():
    a = A()
    codec, _ = tiny_module()
    h = torch.load(os.path.join(GOLDEN_DIR, 'hubert_tiny.pt'), weights_only=True)
    c = h['config']
    w2v = a.HubertWithKmeans.from_state_dict(h['state_dict'], h['centres'], output_layer=c['layers'], conv_feature_layers=c['conv'],
                                             encoder_attention_heads=c['heads'], conv_pos_groups=c['groups']).to(dev())
    wave = rnd(2, 1600, seed=21, scale=0.3).to(dev())
    _, codes, _ = codec(wave, return_encoded=True)
    assert codes.shape == (2, 200, 4)
    sem = a.SemanticTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=w2v.codebook_size, flash_attn=True).to(dev())
    coarse = a.CoarseTransformer(dim=64, depth=1, heads=2, num_semantic_tokens=w2v.codebook_size, codebook_size=32, num_coarse_quantizers=2,
                                 flash_attn=True).to(dev())
    cw = a.CoarseTransformerWrapper(transformer=coarse, codec=codec, wav2vec=w2v, unique_consecutive=False, mask_prob=0.)
    cw.eval()
    la = cw(raw_wave=wave, return_loss=True)
    lb = cw(semantic_token_ids=w2v(wave, flatten=False), coarse_token_ids=codes[..., :2], return_loss=True)
    assert torch.isfinite(la) and float(la.detach()) == float(lb.detach())
    fine = a.FineTransformer(dim=64, depth=1, heads=2, codebook_size=32, num_coarse_quantizers=2, num_fine_quantizers=2, flash_attn=True).to(dev())
    lm = a.AudioLM(wav2vec=w2v, codec=codec, semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    assert lm.coarse.codec is codec and lm.fine.codec is codec
    fw = a.FineTransformerWrapper(transformer=fine, codec=codec)
    out = fw.generate(coarse_token_ids=codes[:1, :8, :2].contiguous(), reconstruct_wave=True)
    assert out.dtype == torch.float32 and out.shape[0] == 1 and out.shape[-1] == 8 * 8 and torch.isfinite(out).all()
