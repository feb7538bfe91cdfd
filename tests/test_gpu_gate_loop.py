"""The gate-loop layers on the MI355X (csrc/gate_loop.hip, codec_bwd.GateLoopFn, soundstream.SoundStream(use_gate_loop_layers=True,
with_gate_loop=True)).

Op level: output and every gradient of one block against float64 CPU autograd of tests/gate_loop_restated.py with a random g, at shapes that sit on
the edges of the scan's chunk (ops.GATE_LOOP_CHUNK), of its 4-step lanes and of the 16-byte path.  In the model: decode(encode(x)) and every parameter
gradient against float64 of the restated stacks; two in-place SGD steps (a stale weight image would show); the neighbours (squeeze-excite, local
attention) run next to it; a model without the switch issues no gate-loop launch.

Tolerance: rel-max <= 2e-5, the project's fp32 conv tolerance (tests/test_gpu_codec_bwd.py).  Measured on the CPU, fp32 eager autograd of the
restatement against float64, sequential and doubling order: at most 7.7e-7 over output and all gradients at the unsaturated shapes.  The
saturated-gate case below ((2, 8, 2 K + 5), the `a` rows of W times 4: long memory across two chunk boundaries) measured the same way: 4.3e-7
(doubling order: y 2.1e-7, dx 3.3e-7, dgamma 1.9e-7, dW 4.3e-7; sequential order: 1.9e-7, 2.4e-7, 3.2e-7, 4.2e-7) -- below one fifth of the bound,
so the scale 4 stays.
Every result is bitwise reproducible (no atomics, a fixed chunk length): two runs are torch.equal."""
import pytest
import torch

import gate_loop_restated as R

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
K = 4096                                                         # ops.GATE_LOOP_CHUNK (asserted below)
OP_SHAPES = [(1, 32, 1), (2, 4, 63), (2, 4, 65), (2, 48, 1001), (1, 512, 70), (1, 8, K - 1), (1, 8, K), (1, 8, K + 1), (2, 8, 3 * K + 17)]
SMALL = dict(channels=4, strides=(2, 4), channel_mults=(2, 4), codebook_dim=16, codebook_size=32, rq_num_quantizers=3, use_local_attn=False)
GL = dict(use_gate_loop_layers=True, with_gate_loop=True)
STACKS = ('encoder.', 'decoder.')


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def check(name, got, ref):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    e = relmax(got, ref)
    print(f'{name}: rel-max {e:.3e}')
    assert e <= TOL, (name, e)


@pytest.fixture(scope='module')
def mods():
    import audiolm_pytorch_amd as A
    from audiolm_pytorch_amd import ops
    assert ops.GATE_LOOP_CHUNK == K
    return A, A.soundstream, ops


# ---------------------------------------------------------------------------------------------- op level

def block_inputs(B, C, T, a_scale=1.0):
    """(x, gamma, W, g): unit-variance x, gamma = 1 + 0.1 randn, W scaled by C^-0.5 (its `a` rows times a_scale)"""
    x, gamma, w, g = rnd(B, C, T, seed=21), 1 + rnd(C, seed=22, scale=0.1), rnd(3 * C, C, seed=23, scale=C ** -0.5), rnd(B, C, T, seed=24)
    w[2 * C:] *= a_scale
    return x, gamma, w, g


def block_reference(x, gamma, w, g):
    """(y, dx, dgamma, dW) by float64 CPU autograd of the restatement"""
    leaves = [t.double().requires_grad_() for t in (x, gamma, w)]
    y = R.gate_loop_block(*leaves)
    y.backward(g.double())
    return (y.detach(),) + tuple(t.grad for t in leaves)


def run_block(S, x, gamma, w, g):
    """the product's block with these parameters: eval-mode output, then twice (training-mode output, dx, dgamma, dW)"""
    B, C, T = x.shape
    block = S.GateLoopBlock(C)
    with torch.no_grad():
        block.fn.fn.norm.gamma.copy_(gamma)
        block.fn.fn.to_qkva[0].weight.copy_(w)
    block.to(dev()).eval()
    with torch.no_grad():
        y_eval = block(x.to(dev()))
    assert y_eval.grad_fn is None
    block.train()
    runs = []
    for _ in range(2):
        block.zero_grad(set_to_none=True)
        xd = x.to(dev()).requires_grad_()
        y = block(xd)
        assert y.grad_fn is not None
        y.backward(g.to(dev()))
        runs.append((y.detach(), xd.grad, block.fn.fn.norm.gamma.grad, block.fn.fn.to_qkva[0].weight.grad))
    return y_eval, runs


def check_block(S, B, C, T, a_scale=1.0):
    inp = block_inputs(B, C, T, a_scale)
    ref = block_reference(*inp)
    y_eval, runs = run_block(S, *inp)
    for name, got, want in zip(('y', 'dx', 'dgamma', 'dW'), runs[0], ref):
        check(f'{name} {(B, C, T)}', got, want)
    assert torch.equal(runs[0][0], y_eval), 'training-mode output differs from the eval-mode output'
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two runs differ'


@pytest.mark.parametrize('B,C,T', OP_SHAPES)
def test_block_forward_backward(mods, B, C, T):
    check_block(mods[1], B, C, T)


def test_block_saturated_gate(mods):
    """the `a` rows of W times 4: the gates sit near 0 and 1, the state remembers across both chunk boundaries (the CPU figures: module docstring)"""
    check_block(mods[1], 2, 8, 2 * K + 5, a_scale=4.)


@pytest.mark.parametrize('B,C,T', [(2, 4, 65), (1, 8, K), (2, 8, K + 3)])
def test_scan_kernels_directly(mods, B, C, T):
    """alm_gate_loop_scan_fwd (both modes) and alm_gate_loop_scan_bwd against the restatement's formulas; the gate's pre-activation at t = 0 gets
    EXACTLY zero"""
    _, _, ops = mods
    x, gamma, w, g = block_inputs(B, C, T)
    _, _, q, kv, a = R.gate_loop_parts(x.double(), gamma.double(), w.double())
    z64 = torch.cat((q, kv, torch.logit(a)), dim=1)
    z = z64.float()
    _, _, _, dz_ref = R.gate_loop_backward(x.double(), gamma.double(), w.double(), g.double())
    zd, xd, gd = z.to(dev()), x.to(dev()), g.to(dev())
    h = ops.gate_loop_scan_fwd(zd)
    zq, zkv, za = z.double().split(C, dim=1)
    h_ref = R.scan_loop(torch.sigmoid(za), zkv)
    check('h', h, h_ref)
    check('y', ops.gate_loop_scan_fwd(zd, xd), zq * h_ref + 2 * x.double())
    dz = ops.gate_loop_scan_bwd(gd, zd, h)
    assert bool((dz[:, 2 * C:, 0] == 0).all()), 'dz_a at t = 0 is not exactly zero'
    for name, lo in (('dq', 0), ('dkv', C), ('dz_a', 2 * C)):
        check(name, dz[:, lo:lo + C], dz_ref[:, lo:lo + C])
    assert torch.equal(dz, ops.gate_loop_scan_bwd(gd, zd, h)) and torch.equal(h, ops.gate_loop_scan_fwd(zd))


def test_norm_kernels_below_the_clamp(mods):
    """an all-zero column: r is the constant sqrt(C) / 1e-12, the output 0 and the gradient finite"""
    _, _, ops = mods
    x = rnd(1, 8, 70, seed=31)
    x[:, :, 5] = 0
    gamma = torch.ones(8)
    xn = ops.gate_loop_norm_fwd(x.to(dev()), gamma.to(dev()))
    assert bool((xn[:, :, 5] == 0).all()) and bool(torch.isfinite(xn).all())
    x64 = x.double().requires_grad_()
    r = (8 ** 0.5) / x64.norm(dim=1, keepdim=True).clamp(min=1e-12)
    (x64 * r).backward(torch.ones_like(x64) * 1e-9)
    dx, _ = ops.gate_loop_norm_bwd(torch.full_like(xn, 1e-9), x.to(dev()), gamma.to(dev()), torch.zeros_like(xn))
    check('dx', dx, x64.grad)


# ---------------------------------------------------------------------------------------------- in the model

def _codec(A, seed=0, **kw):
    torch.manual_seed(seed)
    ss = A.SoundStream(**{**SMALL, **kw})
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in ss.named_parameters():
            if k.endswith('norm.gamma'):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
        for layer in ss.rq.rvqs[0].layers:                       # a trained quantiser's state: the eval-mode forward refuses uninitialised codebooks
            layer._codebook.embed.copy_(torch.randn(layer._codebook.embed.shape, generator=g) * 0.5)
            layer._codebook.initted.fill_(True)
    return ss.to(dev())


def _stack_params(ss):
    return {k: p for k, p in ss.named_parameters() if k.startswith(STACKS)}


def test_model_matches_the_restated_stacks(mods):
    A, _, _ = mods
    ss = _codec(A, **GL)
    x = rnd(2, 1, 512, seed=40, scale=0.5)
    sd64 = {k: p.detach().double().cpu().requires_grad_() for k, p in _stack_params(ss).items()}
    y64 = R.autoencoder(sd64, x.double(), SMALL['strides'])
    y64.square().mean().backward()
    xd = x.to(dev())
    with torch.no_grad():
        y_eval = ss.decode(ss.encode(xd))
    assert y_eval.grad_fn is None
    ss.train()
    runs = []
    for _ in range(2):
        ss.zero_grad(set_to_none=True)
        y = ss.decode(ss.encode(xd))
        assert y.grad_fn is not None
        y.square().mean().backward()
        runs.append({k: p.grad.clone() for k, p in _stack_params(ss).items()})
    assert torch.equal(y.detach(), y_eval), 'training-mode output differs from the eval-mode output'
    check('recon', y.detach(), y64.detach())
    assert set(runs[0]) == set(sd64) and sum('.fn.fn.' in k for k in sd64) == 8
    for k, want in sd64.items():
        check(k, runs[0][k], want.grad)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_two_sgd_steps_pick_up_in_place_updates(mods):
    """an in-place optimiser step must reach the kernels' view of gamma and of to_qkva's weight (its packed images are keyed on the parameter
    version): the third forward follows the restatement's"""
    A, _, _ = mods
    ss = _codec(A, **GL).train()
    x = rnd(1, 1, 512, seed=41, scale=0.5)
    xd = x.to(dev())
    lr = 1e-3                                                    # float64 restatement: the two steps move the output by 23 % and stay stable
    params = _stack_params(ss)
    ref = {k: p.detach().double().cpu() for k, p in params.items()}
    outs, ref_outs = [], []
    for step in range(3):
        p64 = {k: v.clone().requires_grad_() for k, v in ref.items()}
        y64 = R.autoencoder(p64, x.double(), SMALL['strides'])
        ref_outs.append(y64.detach())
        ss.zero_grad(set_to_none=True)
        y = ss.decode(ss.encode(xd))
        outs.append(y.detach())
        if step < 2:
            y64.square().mean().backward()
            ref = {k: (v - lr * p64[k].grad).detach() for k, v in ref.items()}
            y.square().mean().backward()
            with torch.no_grad():
                for p in params.values():
                    p.add_(p.grad, alpha=-lr)
    moved = relmax(ref_outs[2], ref_outs[0])
    print('the two steps move the output by rel-max', moved)
    assert moved > 100 * TOL                                     # far more than the bound: a stale image would show
    for i, (got, want) in enumerate(zip(outs, ref_outs)):
        check(f'recon after {i} steps', got, want)


@pytest.mark.parametrize('kw,wave', [(dict(squeeze_excite=True), 512),
                                     (dict(strides=(2, 4, 5, 8), channel_mults=(2, 4, 8, 16), use_local_attn=True, attn_window_size=64, attn_dim_head=32,
                                           attn_heads=2), 320 * 70)])
def test_neighbours_run_next_to_it(mods, kw, wave):
    """squeeze-excite units, and the local attention of the default use_local_attn=True: forward and backward run, finite, gate-loop gradients nonzero"""
    A, _, _ = mods
    ss = _codec(A, **GL, **kw).train()
    x = rnd(1, 1, wave, seed=42, scale=0.5).to(dev())
    y = ss.decode(ss.encode(x))
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    y.square().mean().backward()
    gate = [(k, p.grad) for k, p in ss.named_parameters() if '.fn.fn.' in k]
    assert len(gate) == 4 * len(ss.strides)
    for k, gr in gate:
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, k


def test_tokenize_and_forward(mods):
    A, _, _ = mods
    ss = _codec(A, **GL)
    wave = rnd(2, 512 + 3, seed=43, scale=0.5).to(dev())
    codes = ss.tokenize(wave)
    assert codes.shape == (1, 2, 64, 3) and codes.dtype == torch.int64 and int(codes.min()) >= 0 and int(codes.max()) < 32
    recon = ss(wave, return_recons_only=True)
    assert recon.shape == (2, 1, 512) and bool(torch.isfinite(recon).all())
    check('decode_from_codebook_indices', ss.decode_from_codebook_indices(codes), recon)


def test_without_the_switch_nothing_changes(mods, monkeypatch):
    """a model built the old way and one built with the opt-in alone (no use_gate_loop_layers): the same state dict, no gate-loop launch, bitwise
    the same outputs"""
    A, _, _ = mods
    from audiolm_pytorch_amd import _lib
    old, new = _codec(A), _codec(A, with_gate_loop=True)
    assert list(old.state_dict()) == list(new.state_dict())
    new.load_state_dict(old.state_dict(), strict=True)
    wave = rnd(2, 512, seed=44, scale=0.5).to(dev())
    want = old(wave, return_recons_only=True), old.tokenize(wave)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = new(wave, return_recons_only=True), new.tokenize(wave)
    assert calls and not [c for c in calls if c.startswith('alm_gate_loop')]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    del calls[:]
    _codec(A, **GL).tokenize(wave)
    assert calls.count('alm_gate_loop_scan_fwd') == 2 and calls.count('alm_gate_loop_norm_fwd') == 2        # the encoder's two blocks
