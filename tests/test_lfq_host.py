"""CPU: the restated residual LFQ (tests/lfq_restated.py) checked against itself in float64 -- index round trip over the whole codebook, the
residual chain, quantize dropout, the grouped layout, the factorised log-sum-exp against the dense softmax, and the closed forms the kernels
implement (losses, dz, parameter gradients) against torch autograd of the dense formulation -- and the host side of the product
(soundstream.GroupedResidualLFQ, SoundStream(use_lookup_free_quantizer=True, with_lfq=True)): constructor checks, module tree, limits, symbols."""
import os
import re

import pytest
import torch

import lfq_restated as R

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS_KW = dict(channels=4, strides=(2, 4, 5, 8), codebook_dim=16, rq_num_quantizers=3, use_local_attn=False)
LFQ_KW = dict(codebook_size=32, use_lookup_free_quantizer=True, with_lfq=True)


@pytest.fixture(scope='module')
def S():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import soundstream
    return soundstream


def relmax(a, b, floor=0.):
    """max |a - b| / max |b|; `floor`: a lower bound of the denominator for a reference that is a difference of two terms which cancel"""
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor, 1e-300)


# ---------------------------------------------------------------------------------------------- the oracle against itself

@pytest.mark.parametrize('d', [1, 5, 10])
def test_oracle_indices_round_trip_over_the_whole_codebook(d):
    idx = torch.arange(2 ** d)
    codes = R.indices_to_codes(idx, d, 0.25)
    assert codes.shape == (2 ** d, d) and set(codes.unique().tolist()) == {-0.25, 0.25}
    assert torch.equal(R.codes_to_indices(codes), idx)
    assert torch.equal(codes, R.codebook(d, 0.25))
    assert len(set(map(tuple, codes.tolist()))) == 2 ** d
    assert int(R.codes_to_indices(torch.zeros(1, d, dtype=F64))) == 0                        # 0 counts as not set
    first = torch.full((d,), -1., dtype=F64)
    first[0] = 1.
    assert int(R.codes_to_indices(first)) == 2 ** (d - 1)                                    # most significant bit first
    assert torch.equal(R.bit_mask(d), torch.tensor([2 ** (d - 1 - j) for j in range(d)]))


def test_oracle_later_layers_never_change_earlier_indices_and_dropout_gives_minus_one():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(100, 5, generator=g, dtype=F64) * 1.5
    cfg = (R.INV_TEMPERATURE, 0.1, 0.25, 1.)
    zsum, idx, losses, rs = R.residual_chain(z, 8, 4, cfg)
    assert rs.shape[0] == 5 and bool((idx[:, 5:] == -1).all()) and bool((idx[:, :5] >= 0).all()) and int(idx.max()) < 32
    assert bool((losses[5:] == 0).all()) and bool((losses[:5] != 0).all())
    grp = R.GroupLFQ(32, 8)
    assert float((grp.decode(idx) - zsum).abs().max()) <= 1e-14
    assert float((grp.decode(idx[:, :5]) - zsum).abs().max()) <= 1e-14
    _, idx_full, losses_full, _ = R.residual_chain(z, 8, 7, cfg)
    assert torch.equal(idx_full[:, :5], idx[:, :5]) and torch.equal(losses_full[:5], losses[:5])
    _, idx_eval, losses_eval, _ = R.residual_chain(z, 8, 7, cfg, train=False)
    assert torch.equal(idx_eval, idx_full) and bool((losses_eval == 0).all())
    # the chain halves the scale: after layer q every residual lies within 2^-q of zero once |z| < 2
    small = z.abs().max(dim=-1).values < 2
    assert float((z - zsum)[small].abs().max()) <= 2. ** -4


def test_oracle_grouped_layout():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 8, generator=g, dtype=F64)
    grouped = R.GroupedLFQ(16, 3, [None, None])
    out, idx, losses, _ = grouped.forward(x, 1)
    assert out.shape == (2, 5, 8) and idx.shape == (2, 2, 5, 3) and losses.shape == (2, 3) and bool((idx[..., 2] == -1).all())
    assert bool((losses[:, 2] == 0).all())
    one = R.GroupLFQ(16, 3)
    o1, i1, l1, *_ = one.forward(x[..., 4:].reshape(10, 4), 1)
    assert torch.equal(out[..., 4:].reshape(10, 4), o1) and torch.equal(idx[1].reshape(10, 3), i1) and torch.equal(losses[1], l1)
    assert float((grouped.decode(idx) - out).abs().max()) <= 1e-14


@pytest.mark.parametrize('d,q', [(1, 0), (4, 0), (5, 3), (10, 0), (10, 7)])
def test_factorised_softmax_equals_the_dense_one(d, q):
    g = torch.Generator().manual_seed(5)
    r = torch.randn(64, d, generator=g, dtype=F64) * 1.5 * 2. ** -q
    s = 2. ** -q
    dense = R.dense_probs(r, d, s)
    p, logp = R.factorised_probs(r, s)
    assert float((p - dense).abs().max()) <= 1e-13 and abs(float(p.sum(dim=-1).max()) - 1) <= 1e-13
    logits = 2 * R.INV_TEMPERATURE * torch.einsum('md,cd->mc', r, R.codebook(d, s))
    assert relmax(R.factorised_lse(r, s), torch.logsumexp(logits, dim=-1)) <= 1e-13
    assert relmax(logp, logits - torch.logsumexp(logits, dim=-1, keepdim=True)) <= 1e-12
    assert bool(torch.isfinite(logp).all())                                                   # logits of several thousand at layer 0: no overflow


CASES = [(64, 24, 32, 3, 2), (1, 12, 1024, 8, 7), (40, 12, 1024, 8, 4), (33, 4, 16, 2, 1), (50, 7, 2, 2, 1), (48, 9, 256, 3, 2)]


@pytest.mark.parametrize('w_c', [0., 0.25])
@pytest.mark.parametrize('M,dim_g,codebook_size,Q,k', CASES, ids=str)
def test_closed_forms_equal_autograd_of_the_dense_formulation(M, dim_g, codebook_size, Q, k, w_c):
    g = torch.Generator().manual_seed(6)
    d = codebook_size.bit_length() - 1
    cfg = (R.INV_TEMPERATURE, 0.1, w_c, 1.)
    ws = None
    if dim_g != d:
        ws = [torch.randn(d, dim_g, generator=g, dtype=F64) * 1.5 / dim_g ** 0.5, torch.randn(d, generator=g, dtype=F64) * 0.1,
              torch.randn(dim_g, d, generator=g, dtype=F64), torch.randn(dim_g, generator=g, dtype=F64)]
        ws = [w.requires_grad_() for w in ws]
    x = (torch.randn(M, dim_g, generator=g, dtype=F64) * (1. if ws else 1.5)).requires_grad_()
    g_out = torch.randn(M, dim_g, generator=g, dtype=F64)
    g_loss = torch.randn(Q, generator=g, dtype=F64)
    grp = R.GroupLFQ(codebook_size, Q, ws, cfg)
    out, idx, losses, z, zsum, rs = grp.forward(x, k)
    ((out * g_out).sum() + (losses * g_loss).sum()).backward()
    wd = None if ws is None else [w.detach() for w in ws]
    c_out, c_losses, c_dx, c_grads = R.closed_form(x.detach(), wd, Q, k, cfg, g_out, g_loss)
    # One token and no commitment term: H(p) - gamma H(mean p) is identically zero at gamma = 1, so the losses and their gradient are a difference of
    # two equal terms; the measure is then relative to the first term (the same run with gamma = 0)
    l_floor = g_floor = 0.
    if M == 1 and w_c == 0:
        _, first, first_dx, _ = R.closed_form(x.detach(), wd, Q, k, (cfg[0], cfg[1], 0., 0.), torch.zeros_like(g_out), g_loss)
        l_floor, g_floor = float(first.abs().max()), float(first_dx.abs().max())
        assert l_floor > 0 and g_floor > 0 and float(losses.detach().abs().max()) <= 1e-11 * l_floor
    assert relmax(c_out, out.detach()) <= 1e-11 and relmax(c_losses, losses.detach(), l_floor) <= 1e-11
    assert relmax(c_dx, x.grad) <= 1e-11
    for got, w in zip(c_grads, ws or []):
        assert relmax(got, w.grad) <= 1e-11
    assert len(c_grads) == (0 if ws is None else 4) and float(x.grad.abs().max()) > 0
    # the loss part alone (it is about 1 % of the whole)
    x2 = x.detach().clone().requires_grad_()
    o2 = R.GroupLFQ(codebook_size, Q, wd, cfg).forward(x2, k)
    (o2[2] * g_loss).sum().backward()
    _, _, l_dx, _ = R.closed_form(x.detach(), wd, Q, k, cfg, torch.zeros_like(g_out), g_loss)
    assert relmax(l_dx, x2.grad, g_floor) <= 1e-11 and (g_floor > 0 or float(x2.grad.abs().max()) > 0)


# ---------------------------------------------------------------------------------------------- the product's host side

def test_constructor_assertions(S):
    with pytest.raises(AssertionError, match='codebook_size'):
        S.SoundStream(**SS_KW, use_lookup_free_quantizer=True, with_lfq=True)                                  # codebook_size missing
    with pytest.raises(AssertionError, match='codebook_size'):
        S.SoundStream(**SS_KW, **LFQ_KW, finite_scalar_quantizer_levels=[4, 3])
    with pytest.raises(AssertionError):
        S.SoundStream(**SS_KW, **LFQ_KW, use_finite_scalar_quantizer=True)
    with pytest.raises(AssertionError, match='power of two'):
        S.SoundStream(**SS_KW, codebook_size=24, use_lookup_free_quantizer=True, with_lfq=True)
    with pytest.raises(AssertionError, match='power of two'):
        S.GroupedResidualLFQ(dim=16, num_quantizers=2, codebook_size=1)
    with pytest.raises(AssertionError):
        S.GroupedResidualLFQ(dim=15, num_quantizers=2, codebook_size=4, groups=2)


def test_lfq_is_refused_without_the_opt_in(S):
    with pytest.raises(NotImplementedError) as e:
        S.SoundStream(**SS_KW, codebook_size=32, use_lookup_free_quantizer=True)
    assert 'LFQ' in str(e.value) and 'with_lfq=True' in str(e.value)
    ss = S.SoundStream(**SS_KW, codebook_size=32, with_lfq=True)                                               # the switch alone changes nothing
    assert isinstance(ss.rq, S.GroupedResidualVQ) and ss.use_lookup_free_quantizer is False


def test_unknown_rq_kwargs_raise_by_name(S):
    for name in ('soft_clamp_input_value', 'frac_per_sample_entropy', 'spherical'):
        with pytest.raises(TypeError, match=name):
            S.SoundStream(**SS_KW, **LFQ_KW, rq_kwargs={name: 1})
    ss = S.SoundStream(**SS_KW, **LFQ_KW, rq_kwargs=dict(quantize_dropout_multiple_of=2, entropy_loss_weight=0.2, commitment_loss_weight=0.25,
                                                         diversity_gamma=2.))
    assert ss.rq.quantize_dropout_multiple_of == 2 and ss.rq.loss_cfg == (100., 0.2, 0.25, 2.)
    assert S.SoundStream(**SS_KW, **LFQ_KW).rq.loss_cfg == (100., 0.1, 0., 1.)


@pytest.mark.parametrize('groups', [1, 2])
def test_module_tree_and_state_dict(S, groups):
    ss = S.SoundStream(**SS_KW, **LFQ_KW, rq_groups=groups)
    assert isinstance(ss.rq, S.GroupedResidualLFQ) and ss.use_lookup_free_quantizer is True and ss.use_finite_scalar_quantizer is False
    assert ss.codebook_size == ss.rq.codebook_size == 32 and ss.rq.codebook_bits == 5 and ss.rq.num_quantizers == 3 and ss.rq.groups == groups
    keys = sorted(k for k in ss.state_dict() if k.startswith('rq.'))
    want = [f'rq.rvqs.{g}.{p}.{t}' for g in range(groups) for p in ('project_in', 'project_out') for t in ('weight', 'bias')]
    want += [f'rq.rvqs.{g}.layers.{q}.mask' for g in range(groups) for q in range(3)]
    assert keys == sorted(want)
    dg = 16 // groups
    assert ss.rq.rvqs[0].project_in.weight.shape == (5, dg) and ss.rq.rvqs[0].project_out.weight.shape == (dg, 5)
    mask = ss.rq.rvqs[0].layers[2].mask
    assert mask.dtype == torch.int64 and mask.tolist() == [16, 8, 4, 2, 1] and torch.equal(mask, R.bit_mask(5))
    assert set(map(id, ss.rq.parameters())) <= set(map(id, ss.non_discr_parameters()))
    ss.load_state_dict(ss.state_dict(), strict=True)


def test_identity_case_has_no_parameters(S):
    rq = S.GroupedResidualLFQ(dim=8, num_quantizers=2, codebook_size=16, groups=2)
    assert list(rq.parameters()) == [] and sorted(rq.state_dict()) == sorted(f'rvqs.{g}.layers.{q}.mask' for g in range(2) for q in range(2))
    assert all(isinstance(r.project_in, torch.nn.Identity) and isinstance(r.project_out, torch.nn.Identity) for r in rq.rvqs)


def test_limits_raise_by_name(S):
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import ops
    assert (ops.LFQ_MAX_CODEBOOK_BITS, ops.LFQ_MAX_DIM, ops.LFQ_MAX_QUANTIZERS) == (10, 1024, 32)
    with pytest.raises(NotImplementedError, match=r'log2\(codebook_size\)'):
        S.GroupedResidualLFQ(dim=64, num_quantizers=2, codebook_size=2048)
    with pytest.raises(NotImplementedError, match='dim / groups'):
        S.GroupedResidualLFQ(dim=2048, num_quantizers=2, codebook_size=16)
    with pytest.raises(NotImplementedError, match='num_quantizers'):
        S.GroupedResidualLFQ(dim=64, num_quantizers=33, codebook_size=16)
    S.GroupedResidualLFQ(dim=2048, num_quantizers=32, codebook_size=1024, groups=2)                            # at the limits


def test_cpu_input_raises(S):
    rq = S.GroupedResidualLFQ(dim=16, num_quantizers=3, codebook_size=32)
    with pytest.raises(RuntimeError):
        rq(torch.zeros(1, 4, 16))
    with pytest.raises(RuntimeError):
        rq.get_output_from_indices(torch.zeros(1, 1, 4, 3, dtype=torch.int64))


def test_training_refuses_more_than_one_rank(S, monkeypatch):
    rq = S.GroupedResidualLFQ(dim=16, num_quantizers=3, codebook_size=32)
    monkeypatch.setattr(torch.distributed, 'is_available', lambda: True)
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a: 2)

    class FakeCuda:                                              # only is_cuda / the check before it are reached
        is_cuda, shape = True, (1, 4, 16)
    with pytest.raises(NotImplementedError, match='GroupedResidualLFQ'):
        rq.train()(FakeCuda())


def test_quantize_dropout_is_the_vq_rule(S):
    import random
    rq = S.GroupedResidualLFQ(dim=16, num_quantizers=8, codebook_size=32, quantize_dropout_cutoff_index=2, quantize_dropout_multiple_of=3)
    vq = S.GroupedResidualVQ(dim=16, num_quantizers=8, codebook_size=4, quantize_dropout_cutoff_index=2, quantize_dropout_multiple_of=3)
    assert S.GroupedResidualLFQ.dropout_index is S.GroupedResidualVQ.dropout_index
    random.seed(5)
    a = [rq.dropout_index() for _ in range(50)]
    random.seed(5)
    assert a == [vq.dropout_index() for _ in range(50)] and set(a) <= {2, 5, 7} and len(set(a)) > 1


def test_symbols_are_declared_bound_and_exported():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import _lib, codec_bwd, ops
    names = ('alm_lfq_fwd_ws_doubles', 'alm_lfq_fwd', 'alm_lfq_decode', 'alm_lfq_bwd_ws_floats', 'alm_lfq_bwd')
    with open(os.path.join(ROOT, 'include', 'audiolm_hip.h')) as fh:
        header = fh.read()
    lib = _lib.load()
    for n in names:
        assert re.search(r'\bint %s\(' % n, header) and n in _lib.SIGNATURES and hasattr(lib, n)
    for n in ('lfq_fwd', 'lfq_decode', 'lfq_bwd', 'LFQ_MAX_CODEBOOK_BITS', 'LFQ_MAX_DIM', 'LFQ_MAX_QUANTIZERS', 'LFQ_INV_TEMPERATURE'):
        assert hasattr(ops, n)
    assert issubclass(codec_bwd.LfqFn, torch.autograd.Function) and ops.LFQ_INV_TEMPERATURE == R.INV_TEMPERATURE
    with open(os.path.join(ROOT, 'audiolm-pytorch_amd', 'build.py')) as fh:
        assert "'lfq.hip'" in fh.read()


def test_workspace_queries_run_on_the_host_and_refuse_the_limits():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import _lib
    assert _lib.query('alm_lfq_fwd_ws_doubles', 100, 10, 8) == 2 * 8 * 1026                  # 2 chunks of 64 rows
    assert _lib.query('alm_lfq_fwd_ws_doubles', 64 * 256 + 1, 5, 2) == 129 * 2 * 34          # chunks doubled to 128 rows
    assert _lib.query('alm_lfq_fwd_ws_doubles', 100, 11, 8) == -1 and _lib.query('alm_lfq_fwd_ws_doubles', 100, 10, 33) == -1
    assert _lib.query('alm_lfq_bwd_ws_floats', 100, 4, 4, 2) == 800                           # identity: the loss gradients only
    assert _lib.query('alm_lfq_bwd_ws_floats', 100, 24, 5, 3) == 1500 + 4 * 272              # + 4 chunks of 32 rows x up4(2 5 24 + 24 + 5)
    assert _lib.query('alm_lfq_bwd_ws_floats', 100, 1025, 5, 3) == -1 and _lib.query('alm_lfq_bwd_ws_floats', 100, 24, 11, 3) == -1
