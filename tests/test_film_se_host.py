"""CPU: the host side of the denoising SoundStream (csrc/film_se.hip, soundstream.FiLM / SqueezeExcite): the restatement tests/film_se_restated.py
against the REAL reference's fixture tests/golden/film_se_small.pt, module tree and state-dict names, the parameter order, the refusals and the
workspace arithmetic.  No launch: there is no GPU here."""
import os

import pytest
import torch
import torch.nn.functional as F

import film_se_restated as R
from common import GOLDEN_DIR, synth_state_dict

import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib, ops, soundstream as S

PREFIXES = ('encoder.', 'decoder.', 'encoder_film.', 'decoder_film.')
SMALL = dict(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, use_local_attn=False)


@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'film_se_small.pt'), weights_only=False)
    return fx, synth_state_dict(fx['shapes'], fx['seed'])


def test_restatement_reproduces_the_reference(golden):
    """loss to 1e-5, reconstruction and every gradient to rel-max 2e-5, for both conditions, in fp32 on the CPU like the fixture"""
    fx, sd0 = golden
    wave = fx['inputs']['wave']
    x = wave[:, None, :wave.shape[-1] // 320 * 320]
    for name, is_denoising in (('denoise', True), ('plain', False)):
        sd = {k: v.clone().requires_grad_() for k, v in sd0.items()}
        y = R.denoising_autoencoder(sd, x, is_denoising, strides=tuple(fx['ctor']['strides']))
        loss = F.mse_loss(y, x)
        loss.backward()
        ref = fx['outputs'][name]
        assert abs(float(loss.detach()) - float(ref['loss'])) <= 1e-5 * abs(float(ref['loss']))
        assert float((y.detach() - ref['recon']).abs().max()) <= 2e-5 * float(ref['recon'].abs().max())
        grads = R.golden_grads(ref)
        assert set(grads) == set(sd0) and len(grads) == 220
        for k, (shape, stride, want) in grads.items():
            got = sd[k].grad
            assert got is not None and tuple(got.shape) == shape, k
            assert float((got.reshape(-1)[::stride] - want).abs().max()) <= 2e-5 * float(want.abs().max()), k
        col = 1 if is_denoising else 0                           # the condition's zero entry silences one column of each to_cond.weight gradient
        for film in ('encoder_film', 'decoder_film'):
            g = sd[f'{film}.to_cond.weight'].grad
            assert float(g[:, col].abs().max()) == 0 and float(g[:, 1 - col].abs().max()) > 0


def test_cumulative_mean_runs_over_channels():
    u = torch.arange(24.).reshape(1, 4, 6)
    m = R.channel_cumulative_mean(u)
    L = torch.tril(torch.ones(4, 4)) / torch.arange(1., 5.)[:, None]
    assert torch.allclose(m, torch.einsum('dc,bcn->bdn', L, u))
    assert torch.equal(m[0, 0], u[0, 0]) and torch.allclose(m[0, 3], u[0].mean(0))


def test_module_tree_and_state_dict_match_the_reference(golden):
    fx, sd = golden
    ss = A.SoundStream(**fx['ctor'], with_film=True)
    ours = {k: tuple(v.shape) for k, v in ss.state_dict().items() if k.startswith(PREFIXES)}
    assert ours == {k: tuple(v) for k, v in fx['shapes'].items()}
    assert all(k.startswith(PREFIXES + ('rq.',)) for k in ss.state_dict())
    unit = ss.encoder[1][0]
    assert [type(m).__name__ for m in unit.fn] == ['CausalConv1d', 'ELU', 'CausalConv1d', 'ELU', 'SqueezeExcite']
    assert tuple(ss.encoder[4][0].fn[4].net[0].weight.shape) == (8, 32, 1) and tuple(ss.encoder[4][0].fn[4].net[2].weight.shape) == (32, 8, 1)
    assert tuple(ss.encoder_film.to_cond.weight.shape) == (32, 2) and tuple(ss.decoder_film.to_cond.bias.shape) == (32,)
    full = dict(ss.state_dict())
    full.update(sd)
    ss.load_state_dict(full, strict=True)
    assert torch.equal(ss.decoder_film.to_cond.weight, sd['decoder_film.to_cond.weight'])
    assert S.SqueezeExcite(256).net[0].out_channels == 64 and S.SqueezeExcite(12).net[0].out_channels == 8
    fresh = A.SoundStream(**SMALL, with_film=True).decoder_film.to_cond                        # nn.Linear default init: |w|, |b| <= 1 / sqrt(fan_in = 2)
    assert isinstance(fresh, torch.nn.Linear) and max(float(fresh.weight.detach().abs().max()), float(fresh.bias.detach().abs().max())) <= 2 ** -0.5 + 1e-6
    one = S.ResidualUnit(8, 8, 3, squeeze_excite=True)
    assert sorted(one.state_dict()) == ['fn.0.conv.bias', 'fn.0.conv.weight', 'fn.2.conv.bias', 'fn.2.conv.weight', 'fn.4.net.0.bias', 'fn.4.net.0.weight',
                                        'fn.4.net.2.bias', 'fn.4.net.2.weight']


def test_non_discr_parameters_order():
    """the reference's order (soundstream.py:760-769): encoder, decoder, the attention blocks, the two FiLMs, rq -- each parameter exactly once"""
    ss = A.SoundStream(codebook_size=32, codebook_dim=64, channels=4, attn_dim_head=32, attn_heads=2, attn_window_size=16, with_film=True,
                       squeeze_excite=True)
    names = {id(p): n for n, p in ss.named_parameters()}
    got = [names[id(p)] for p in ss.non_discr_parameters()]
    assert len(got) == len(set(got)) == len(list(ss.parameters()))
    heads = []
    for n in got:
        top = n.split('.')[0]
        if not heads or heads[-1] != top:
            heads.append(top)
    assert heads == ['encoder', 'decoder', 'encoder_attn', 'decoder_attn', 'encoder_film', 'decoder_film']      # rq holds buffers only
    assert got[-4:] == ['encoder_film.to_cond.weight', 'encoder_film.to_cond.bias', 'decoder_film.to_cond.weight', 'decoder_film.to_cond.bias']
    plain = A.SoundStream(**SMALL, squeeze_excite=True)
    assert not hasattr(plain, 'encoder_film') and len(plain.non_discr_parameters()) == len(list(plain.parameters()))
    assert sum('fn.4.net' in n for n, _ in plain.named_parameters()) == 24 * 4


def test_refusals():
    x = torch.zeros(1, 640)
    plain = A.SoundStream(**SMALL)
    with pytest.raises(NotImplementedError, match='with_discriminators=True'):
        plain(x, target=x, is_denoising=True, return_recons_only=True)
    no_film = A.SoundStream(**SMALL, multi_spectral_recon_loss_weight=0., stft_discriminator=False, with_discriminators=True)
    with pytest.raises(NotImplementedError, match='is_denoising'):
        no_film(x, target=x, is_denoising=False)
    film = A.SoundStream(**SMALL, with_film=True, squeeze_excite=True)
    with pytest.raises(AssertionError, match='target'):
        film(x, is_denoising=True, return_recons_only=True)
    with pytest.raises(NotImplementedError, match='with_discriminators=True'):        # the loss branches stay opt-in
        film(x, target=x, is_denoising=True)
    for kw in (dict(return_recons_only=True), dict(return_encoded=True), dict(return_codes_only=True)):
        with pytest.raises(RuntimeError, match='MI355X only'):                        # past the option checks the CPU is refused, as everywhere
            film(x, target=x, is_denoising=True, **kw)
    with pytest.raises(NotImplementedError, match='squeeze_excite'):                  # 1024 channels -> hidden width 256: by name, at construction
        S.ResidualUnit(1024, 1024, 1, squeeze_excite=True)
    with pytest.raises(NotImplementedError, match='squeeze_excite'):
        A.SoundStream(codebook_size=32, channels=128, squeeze_excite=True)
    with pytest.raises(NotImplementedError, match='gate-loop'):
        A.SoundStream(**SMALL, use_gate_loop_layers=True)
    with pytest.raises(NotImplementedError, match='stochastic'):
        A.SoundStream(**SMALL, rq_stochastic_sample_codes=True)
    with pytest.raises(RuntimeError, match='MI355X only'):
        S.SqueezeExcite(8)(torch.zeros(1, 8, 4))
    with pytest.raises(RuntimeError, match='MI355X only'):
        S.FiLM(8)(torch.zeros(1, 4, 8), (1., 0.))


def test_wrappers_refuse_cpu_tensors():
    u, w1, b1, w2, b2 = torch.zeros(1, 8, 4), torch.zeros(8, 8, 1), torch.zeros(8), torch.zeros(8, 8, 1), torch.zeros(8)
    with pytest.raises(_lib.AlmError):
        ops.se_gate_fwd(u, w1, b1, w2, b2)
    with pytest.raises(_lib.AlmError):
        ops.se_gate_bwd(u, u, w1, b1, w2, b2)
    x, w, b = torch.zeros(3, 8), torch.zeros(16, 2), torch.zeros(16)
    with pytest.raises(_lib.AlmError):
        ops.film_fwd(x, w, b, 1., 0.)
    with pytest.raises(_lib.AlmError):
        ops.film_bwd(x, x, w, b, 1., 0.)


def test_workspace_queries():
    """alm_se_gate_bwd keeps m, dz2 [B][C][T] and h, dz1 [B][inner][T] plus the workspaces of its two k = 1 weight-gradient calls; alm_film_bwd
    keeps 2 C partial sums per row chunk (32 rows, doubled until at most 1024 chunks); both are functions of the shapes alone"""
    up4 = lambda n: -(-n // 4) * 4                               # noqa: E731
    q = lambda *a: _lib.query('alm_se_gate_bwd_ws_floats', *a)   # noqa: E731
    for B, C, inner, T in ((2, 4, 8, 333), (1, 32, 8, 1), (2, 48, 12, 1000), (1, 256, 64, 130), (1, 512, 128, 70), (2, 32, 8, 4099), (8, 32, 8, 80000)):
        w1 = _lib.query('alm_conv1d_wgrad_ws_floats', B, C, inner, T, 1)
        w2 = _lib.query('alm_conv1d_wgrad_ws_floats', B, inner, C, T, 1)
        assert w1 > 0 and w2 > 0
        assert q(B, C, inner, T) == 2 * up4(B * C * T) + 2 * up4(B * inner * T) + up4(w1) + up4(w2) == q(B, C, inner, T)
    assert q(1, 1024, 256, 64) == -1 and q(1, 512, 129, 64) == -1                     # outside the envelope
    assert q(8, 512, 128, 1 << 20) == -1                                              # past 2^31 floats
    assert ops.se_gate_supported(512, 128) and ops.se_gate_supported(1, 8) and ops.se_gate_supported(4, 8)
    assert not ops.se_gate_supported(1024, 256) and not ops.se_gate_supported(0, 8)
    f = lambda *a: _lib.query('alm_film_bwd_ws_floats', *a)      # noqa: E731
    assert f(14, 16) == 1 * 2 * 16 and f(1, 512) == 2 * 512 and f(3000, 96) == 94 * 2 * 96
    assert f(32 * 1024, 8) == 1024 * 2 * 8 and f(32 * 1024 + 1, 8) == 513 * 2 * 8     # the chunk doubles past 1024 chunks
