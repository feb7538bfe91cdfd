"""CPU: the restated gate-loop layer (tests/gate_loop_restated.py) checked against itself in float64 -- the sequential scan against the log-step
doubling, the analytic backward formulas the kernels implement against torch autograd -- and the host side of the product
(SoundStream(use_gate_loop_layers=True, with_gate_loop=True)): module tree, state-dict keys, strict load, refusals, limits, symbols."""
import pytest
import torch

import gate_loop_restated as R

F32, F64 = torch.float32, torch.float64
SMALL = dict(channels=4, strides=(2, 4), channel_mults=(2, 4), codebook_dim=16, codebook_size=32, rq_num_quantizers=3, use_local_attn=False)
GL = dict(use_gate_loop_layers=True, with_gate_loop=True)


@pytest.fixture(scope='module')
def A():
    import audiolm_pytorch_amd
    return audiolm_pytorch_amd


def rnd(*shape, seed=0, scale=1.0, dtype=F64):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype) * scale


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def inputs(B, C, T, a_scale=1.0):
    x, gamma, w, g = rnd(B, C, T, seed=1), 1 + rnd(C, seed=2, scale=0.1), rnd(3 * C, C, seed=3, scale=C ** -0.5), rnd(B, C, T, seed=4)
    w[2 * C:] *= a_scale
    return x, gamma, w, g


# ---------------------------------------------------------------------------------------------- the restatement against itself

@pytest.mark.parametrize('B,C,T', [(1, 3, 1), (2, 4, 2), (2, 5, 63), (1, 8, 64), (2, 3, 333)])
def test_loop_scan_equals_doubling_scan(B, C, T):
    a, kv = torch.sigmoid(rnd(B, C, T, seed=5, scale=2.)), rnd(B, C, T, seed=6)
    loop, dbl = R.scan_loop(a, kv), R.scan_doubling(a, kv)
    assert loop.shape == (B, C, T) and relmax(dbl, loop) <= 1e-13
    a2 = a.clone()
    a2[..., 0] = 0.123                                           # a[0] is unused by both forms
    assert torch.equal(R.scan_loop(a2, kv), loop) and torch.equal(R.scan_doubling(a2, kv), dbl)
    x, gamma, w, _ = inputs(B, C, T)
    assert relmax(R.gate_loop_block(x, gamma, w, scan=R.scan_loop), R.gate_loop_block(x, gamma, w, scan=R.scan_doubling)) <= 1e-13


def test_block_formula_by_hand():
    """c = 1, n = 3 worked by hand: the RMSNorm of one channel is sign(x), the skips add 2 x"""
    x = torch.tensor([[[2., -3., 0.5]]], dtype=F64)
    gamma, w = torch.tensor([1.5], dtype=F64), torch.tensor([[2.], [1.], [0.5]], dtype=F64)
    xn = torch.tensor([1.5, -1.5, 1.5], dtype=F64)
    q, kv, a = 2 * xn, xn, torch.sigmoid(0.5 * xn)
    h0 = kv[0]
    h1 = a[1] * h0 + kv[1]
    h2 = a[2] * h1 + kv[2]
    want = q * torch.stack((h0, h1, h2)) + 2 * x[0, 0]
    assert relmax(R.gate_loop_block(x, gamma, w)[0, 0], want) <= 1e-15


@pytest.mark.parametrize('B,C,T,a_scale', [(1, 3, 1, 1.), (2, 4, 7, 1.), (2, 6, 130, 1.), (1, 5, 97, 4.)])
def test_analytic_backward_equals_autograd(B, C, T, a_scale):
    x, gamma, w, g = inputs(B, C, T, a_scale)
    leaves = [t.clone().requires_grad_() for t in (x, gamma, w)]
    R.gate_loop_block(*leaves, scan=R.scan_loop).backward(g)
    dx, dgamma, dw, dz = R.gate_loop_backward(x, gamma, w, g)
    for name, got, want in zip(('dx', 'dgamma', 'dW'), (dx, dgamma, dw), (t.grad for t in leaves)):
        assert relmax(got, want) <= 1e-12, name
    assert bool((dz[:, 2 * C:, 0] == 0).all())                   # the gate's pre-activation at t = 0 gets exactly nothing


def test_stacks_place_the_blocks_like_the_module_tree(A):
    """the restated stacks read exactly the keys of the product's state dict (every encoder / decoder entry is used: a gradient reaches it)"""
    ss = A.SoundStream(**SMALL, **GL)
    sd = {k: v.detach().double().clone().requires_grad_() for k, v in ss.state_dict().items() if k.startswith(('encoder.', 'decoder.'))}
    x = rnd(1, 1, 512, seed=9)                                   # 64 frames after the strides: every reflect pad (up to 54) fits
    y = R.autoencoder(sd, x, strides=SMALL['strides'])
    assert y.shape == x.shape
    y.square().mean().backward()
    assert all(v.grad is not None and float(v.grad.abs().max()) > 0 for v in sd.values())


# ---------------------------------------------------------------------------------------------- the product's host side

def gate_keys(prefix, indices):
    return [f'{prefix}.{i}.fn.fn.{leaf}' for i in indices for leaf in ('norm.gamma', 'to_qkva.0.weight')]


def test_module_tree_and_keys_small(A):
    S = A.soundstream
    ss = A.SoundStream(**SMALL, **GL)
    assert len(ss.encoder) == 6 and len(ss.decoder) == 6
    for stack in (ss.encoder, ss.decoder):
        assert [type(m).__name__ for m in stack] == ['CausalConv1d', 'Sequential', 'Residual', 'Sequential', 'Residual', 'CausalConv1d']
        for m in (stack[2], stack[4]):
            assert isinstance(m, S.Residual) and isinstance(m.fn, S.ChannelTranspose) and isinstance(m.fn.fn, S.SimpleGateLoopLayer)
    sd = ss.state_dict()
    got = sorted(k for k in sd if '.fn.fn.' in k)
    assert got == sorted(gate_keys('encoder', (2, 4)) + gate_keys('decoder', (2, 4)))
    dims = {'encoder.2': 8, 'encoder.4': 16, 'decoder.2': 8, 'decoder.4': 4}                  # encoder: chan_out of its block; decoder: chan_in
    for p, c in dims.items():
        assert tuple(sd[p + '.fn.fn.norm.gamma'].shape) == (c,) and tuple(sd[p + '.fn.fn.to_qkva.0.weight'].shape) == (3 * c, c)
        assert bool((sd[p + '.fn.fn.norm.gamma'] == 1).all())
        assert float(sd[p + '.fn.fn.to_qkva.0.weight'].abs().max()) <= c ** -0.5 + 1e-6          # nn.Linear default init
    assert 'encoder.5.conv.weight' in sd and 'decoder.5.conv.weight' in sd                    # the final convs move up
    plain = A.SoundStream(**SMALL)
    assert not any('.fn.fn.' in k for k in plain.state_dict()) and len(plain.encoder) == 4 and 'encoder.3.conv.weight' in plain.state_dict()


def test_module_tree_and_keys_default(A):
    ss = A.SoundStream(codebook_size=64, rq_num_quantizers=2, **GL)
    sd = ss.state_dict()
    got = sorted(k for k in sd if '.fn.fn.' in k)
    assert got == sorted(gate_keys('encoder', (2, 4, 6, 8)) + gate_keys('decoder', (2, 4, 6, 8)))
    assert [sd[f'encoder.{i}.fn.fn.norm.gamma'].shape[0] for i in (2, 4, 6, 8)] == [64, 128, 256, 512]
    assert [sd[f'decoder.{i}.fn.fn.norm.gamma'].shape[0] for i in (2, 4, 6, 8)] == [256, 128, 64, 32]
    assert [tuple(sd[f'decoder.{i}.fn.fn.to_qkva.0.weight'].shape) for i in (2, 8)] == [(768, 256), (96, 32)]
    assert 'encoder.9.conv.weight' in sd and 'decoder.9.conv.weight' in sd and len(ss.encoder) == 10 and len(ss.decoder) == 10
    assert ss.encoder_attn is not None                           # the local attention stays next to it


def test_strict_load_of_a_reference_layout_state_dict(A):
    ss = A.SoundStream(**SMALL, **GL)
    synth = {k: rnd(*v.shape, seed=i, dtype=F32) if v.is_floating_point() else v.clone() for i, (k, v) in enumerate(ss.state_dict().items())}
    other = A.SoundStream(**SMALL, **GL)
    other.load_state_dict(synth, strict=True)
    assert torch.equal(other.encoder[2].fn.fn.norm.gamma, synth['encoder.2.fn.fn.norm.gamma'])
    assert torch.equal(other.decoder[4].fn.fn.to_qkva[0].weight, synth['decoder.4.fn.fn.to_qkva.0.weight'])
    with pytest.raises(RuntimeError, match='fn.fn'):             # a checkpoint without the layers does not load strictly
        other.load_state_dict(A.SoundStream(**SMALL).state_dict(), strict=True)


def test_parameters_are_generator_parameters(A):
    ss = A.SoundStream(**SMALL, **GL)
    ids = {id(p) for p in ss.non_discr_parameters()}
    gate = [p for n, p in ss.named_parameters() if '.fn.fn.' in n]
    assert len(gate) == 8 and all(id(p) in ids for p in gate)
    assert len(ss.non_discr_parameters()) == len(list(ss.parameters()))


def test_refusals(A):
    S = A.soundstream
    with pytest.raises(NotImplementedError, match='gate-loop.*with_gate_loop=True'):
        A.SoundStream(**SMALL, use_gate_loop_layers=True)
    with pytest.raises(NotImplementedError, match='stochastic'):
        A.SoundStream(**SMALL, rq_stochastic_sample_codes=True)
    with pytest.raises(NotImplementedError, match='stochastic'):
        A.SoundStream(**SMALL, rq_stochastic_sample_codes=True, **GL)
    assert not any('.fn.fn.' in k for k in A.SoundStream(**SMALL, with_gate_loop=True).state_dict())      # the opt-in alone builds nothing
    ss = A.SoundStream(**SMALL, **GL)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ss.encoder[2](torch.zeros(1, 8, 5))
    with pytest.raises(RuntimeError, match='MI355X only'):
        ss.encode(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match='MI355X only'):
        ss.decode(torch.zeros(1, 4, 16))
    with pytest.raises(NotImplementedError, match='cache'):
        ss.encoder[2](torch.zeros(1, 8, 5), cache=None)
    with pytest.raises(NotImplementedError, match='return_cache'):
        ss.encoder[2].fn.fn(torch.zeros(1, 5, 8), return_cache=True)
    with pytest.raises(NotImplementedError, match='post_ln'):
        S.SimpleGateLoopLayer(8, post_ln=True)
    with pytest.raises(NotImplementedError, match='reverse'):
        S.SimpleGateLoopLayer(8, reverse=True)
    with pytest.raises(NotImplementedError, match='Residual'):
        S.Residual(torch.nn.Identity())


def test_ops_refuse_cpu_tensors_and_the_chunk_is_the_librarys(A):
    from audiolm_pytorch_amd import _lib, ops
    assert ops.GATE_LOOP_CHUNK == _lib.query('alm_gate_loop_chunk') == 4096
    x, gamma, z = torch.zeros(1, 4, 8), torch.ones(4), torch.zeros(1, 12, 8)
    with pytest.raises(_lib.AlmError):
        ops.gate_loop_norm_fwd(x, gamma)
    with pytest.raises(_lib.AlmError):
        ops.gate_loop_scan_fwd(z, x)
    with pytest.raises(_lib.AlmError):
        ops.gate_loop_scan_bwd(x, z, x)
    with pytest.raises(_lib.AlmError):
        ops.gate_loop_norm_bwd(x, x, gamma, x)


def test_launchers_validate_before_launching(A):
    """host arithmetic only: the size queries, and NULL pointers / bad shapes come back as the library's error codes without a launch"""
    from audiolm_pytorch_amd import _lib
    K = 4096
    q = lambda *a: _lib.query('alm_gate_loop_scan_ws_floats', *a)
    assert q(2, 8, 1) == 0 and q(2, 8, K) == 0 and q(2, 8, K + 1) == 3 * 16 * 2 and q(1, 32, 3 * K + 17) == 3 * 32 * 4
    assert q(65535, 512, 1 << 20) == -1
    assert _lib.query('alm_gate_loop_norm_bwd_ws_floats', 2, 8, 513) == 2 * 2 * 8
    assert _lib.query('alm_gate_loop_norm_bwd_ws_floats', 1 << 15, 1 << 15, 1 << 15) == -1
    bad, unsupported = 10001, 10002
    assert _lib.query('alm_gate_loop_norm_fwd', None, None, None, 1, 4, 8, None) == bad
    assert _lib.query('alm_gate_loop_scan_fwd', None, None, None, None, 0, 1, 4, 8, 0, None) == bad
    assert _lib.query('alm_gate_loop_scan_bwd', None, None, None, None, None, 0, 1, 4, 8, None) == bad
    assert _lib.query('alm_gate_loop_norm_bwd', None, None, None, None, None, None, None, 0, 1, 4, 8, None) == bad
    one = 16                                                     # a non-NULL address that is never dereferenced: validation comes first
    assert _lib.query('alm_gate_loop_norm_fwd', one, one, one, 1, 0, 8, None) == bad
    assert _lib.query('alm_gate_loop_norm_fwd', one, one, one, 65536, 4, 8, None) == unsupported
    assert _lib.query('alm_gate_loop_scan_fwd', one, one, one, None, 0, 1, 4, K + 1, 0, None) == bad          # multi-chunk rows need the workspace
    assert _lib.query('alm_gate_loop_scan_fwd', one, one, one, one, 10, 1, 4, K + 1, 0, None) == bad          # ... of the right size
    assert _lib.query('alm_gate_loop_scan_fwd', one, one, one, one, 1 << 40, 65535, 512, 1 << 20, 0, None) == unsupported
    assert _lib.query('alm_gate_loop_scan_bwd', one, one, one, one, None, 0, 1, 4, K + 1, None) == bad
    assert _lib.query('alm_gate_loop_norm_bwd', one, one, one, one, one, one, one, 3, 1, 4, 8, None) == bad
