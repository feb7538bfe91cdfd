"""Backward of SoundStream's LocalTransformer on the MI355X (csrc/local_attn_bwd.hip + the autograd Functions of audiolm_pytorch_amd/codec_bwd.py).

Op level: dqkv / dgates / dq_scale / dk_scale of the windowed attention, LayerNorm and GEGLU backward against float64 CPU autograd.
Block level: dx and every parameter gradient of LocalTransformer against float64 autograd of the restated library (oracle/local_attention_restated.py).
End to end: loss and every gradient of the default-constructor SoundStream against the REAL reference (tests/golden/codec_bwd_local_attn_small.pt),
and two in-place SGD steps against the float64 restatement (weight-image invalidation).

Metric: rel-max, max|a - b| / max|b|.  Bound: TOL = 4e-5 at every specified shape, the bound the block was specified with.  Measured on the CPU at the
shapes below, fp32 autograd of the reference formulation against float64 autograd of it deviates by at most (worst over the shapes of each group)
    attention op     dqkv 3.8e-6, dgates 1.9e-6, dq_scale 3.3e-6, dk_scale 5.9e-6 (six specified shapes; the two added ones: ATTN_TOL)
    LayerNorm        dx 1.4e-7, dgamma 2.1e-7, dbeta 2.1e-7;   GEGLU du 1.1e-7
    whole block      dx 9.4e-7, parameters 2.8e-6 (k_scale of layer 0 at depth 2, T = 129)
    end to end       loss 8.5e-8, parameters 5.4e-6 (the fp32 golden against the float64 restatement; worst: decoder.4.0.conv.bias)
Ten times the block figures stays under TOL.  Ten times the attention-op and end-to-end figures (5.9e-5, 5.4e-5) would allow a wider bound for those
tests; TOL is kept for them all the same (6.8x resp. 7.4x the reference's own fp32 error).  Every parameter gradient of the reference is non-zero at
these shapes (check() asserts it).  Every gradient is bitwise reproducible (no atomics): two runs are torch.equal.  One SGD step at lr 1e-4 moves
the float64 loss by 1.4e-2 relative."""
import os

import pytest
import torch
import torch.nn.functional as F

import local_attention_restated as LR
from common import GOLDEN_DIR, synth_state_dict

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 4e-5


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def check(name, got, ref, tol=TOL):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert float(ref.abs().max()) > 0, name
    e = relmax(got, ref)
    print(f'{name}: rel-max {e:.3e}')
    assert e <= tol, (name, e)


@pytest.fixture(scope='module')
def ops():
    from audiolm_pytorch_amd import ops as _ops
    return _ops


def _mods():
    from audiolm_pytorch_amd import soundstream as S
    return S


# ---------------------------------------------------------------------------------------------- 1. the attention op

ATTN_SHAPES = [(2, 2, 32, 129, 64), (1, 3, 32, 64, 64), (2, 2, 32, 40, 64), (2, 2, 32, 50, 16), (1, 8, 64, 300, 128), (1, 2, 64, 257, 128),
               (1, 1, 64, 170, 160), (1, 2, 32, 260, 256)]      # + the widest windows: dh 64 where lse / delta leave the LDS, dh 32 at 256 threads


# The two added shapes have larger CPU fp32-vs-float64 deviations than the specified ones (longest windows: 257 scores per row); where ten times the
# measured deviation exceeds TOL, that product is the bound of that tensor at that shape (measured: dqkv 4.77e-6, dk_scale 4.52e-6; dqkv 9.87e-6).
ATTN_TOL = {(1, 1, 64, 170, 160): dict(dqkv=4.8e-5, dk_scale=4.6e-5), (1, 2, 32, 260, 256): dict(dqkv=9.9e-5)}


def attn_inputs(B, H, dh, T, W):
    return dict(qkv=rnd(B, 3 * H * dh, T, seed=1), gates=rnd(B, H, T, seed=2), do=rnd(B, H * dh, T, seed=3),
                q_scale=1.0 + 0.3 * rnd(dh, seed=4), k_scale=1.0 + 0.3 * rnd(dh, seed=5))


def attn_ref(inp, B, H, dh, T, W, dtype=F64):
    """autograd of l2norm * scale -> LocalAttention (restated library) -> sigmoid gate: (dqkv, dgates, dq_scale, dk_scale)"""
    leaf = {k: inp[k].detach().clone().to(dtype).requires_grad_() for k in ('qkv', 'gates', 'q_scale', 'k_scale')}
    q, k, v = (t.transpose(-1, -2) for t in leaf['qkv'].view(B, 3, H, dh, T).unbind(1))            # [B, H, T, dh]
    q, k = LR.l2norm(q) * leaf['q_scale'], LR.l2norm(k) * leaf['k_scale']
    attn = LR.LocalAttention(dim=dh, window_size=W, causal=True, autopad=True, scale=8, exact_windowsize=True, use_xpos=True).to(dtype)
    out = attn(q, k, v) * leaf['gates'].sigmoid()[..., None]
    out.transpose(-1, -2).reshape(B, H * dh, T).backward(inp['do'].to(dtype))
    return tuple(leaf[k].grad for k in ('qkv', 'gates', 'q_scale', 'k_scale'))


def attn_gpu(ops, inp, B, H, dh, T, W):
    S = _mods()
    d = {k: v.to(dev()).contiguous() for k, v in inp.items()}
    tabs = S._SinusoidalEmbeddings(dh, scale_base=W // 2).tables(2 * W, dev())
    o = ops.local_attn(d['qkv'], d['q_scale'], d['k_scale'], *tabs, d['gates'], H, dh, W, 8)
    return ops.local_attn_bwd(d['qkv'], d['q_scale'], d['k_scale'], *tabs, d['gates'], o, d['do'], H, dh, W, 8)


@pytest.mark.parametrize('B,H,dh,T,W', ATTN_SHAPES)
def test_attention_backward(ops, B, H, dh, T, W):
    inp = attn_inputs(B, H, dh, T, W)
    ref = attn_ref(inp, B, H, dh, T, W)
    got = attn_gpu(ops, inp, B, H, dh, T, W)
    for name, g, r in zip(('dqkv', 'dgates', 'dq_scale', 'dk_scale'), got, ref):
        check(name, g, r, ATTN_TOL.get((B, H, dh, T, W), {}).get(name, TOL))
    again = attn_gpu(ops, inp, B, H, dh, T, W)
    assert all(torch.equal(a, c) for a, c in zip(got, again))


# ---------------------------------------------------------------------------------------------- 2. LayerNorm / GEGLU backward

@pytest.mark.parametrize('B,C,T', [(2, 48, 300), (1, 50, 257)])
@pytest.mark.parametrize('with_residual', [False, True])
def test_layernorm_backward(ops, B, C, T, with_residual):
    x, dy, gamma, beta, res = rnd(B, C, T, seed=1), rnd(B, C, T, seed=2), 1.0 + 0.3 * rnd(C, seed=3), 0.2 * rnd(C, seed=4), rnd(B, C, T, seed=5)
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
    F.layer_norm(x64.transpose(1, 2), (C,), g64, b64, 1e-5).transpose(1, 2).backward(dy.double())
    rdx = x64.grad + res.double() if with_residual else x64.grad
    run = lambda: ops.layernorm_bct_bwd(dy.to(dev()), x.to(dev()), gamma.to(dev()), 1e-5, residual=res.to(dev()) if with_residual else None)
    dx, dgamma, dbeta = run()
    check('dx', dx, rdx), check('dgamma', dgamma, g64.grad), check('dbeta', dbeta, b64.grad)
    assert all(torch.equal(a, c) for a, c in zip((dx, dgamma, dbeta), run()))
    dx2, none_g, none_b = ops.layernorm_bct_bwd(dy.to(dev()), x.to(dev()), gamma.to(dev()), 1e-5, residual=res.to(dev()) if with_residual else None,
                                                need_params=False)
    assert none_g is None and none_b is None and torch.equal(dx2, dx)


def test_geglu_backward(ops):
    B, I, T = 2, 85, 131
    u, dh = rnd(B, 2 * I, T, seed=1), rnd(B, I, T, seed=2)
    u64 = u.double().requires_grad_()
    a, gate = u64.chunk(2, dim=1)
    (a * F.gelu(gate)).backward(dh.double())
    du = ops.geglu_bct_bwd(dh.to(dev()), u.to(dev()))
    check('du', du, u64.grad)
    assert torch.equal(du, ops.geglu_bct_bwd(dh.to(dev()), u.to(dev())))


# ---------------------------------------------------------------------------------------------- 3. the whole block

class RefLocalTransformer(torch.nn.Module):                         # = the reference's own LocalTransformer.forward (soundstream.py:397-440)
    def __init__(self, dim, heads, dh, W, depth):
        super().__init__()
        self.layers = torch.nn.ModuleList([torch.nn.ModuleList([
            LR.LocalMHA(dim=dim, heads=heads, dim_head=dh, qk_rmsnorm=True, window_size=W, use_rotary_pos_emb=True, gate_values_per_head=True,
                        use_xpos=True, prenorm=True, causal=True), LR.FeedForward(dim=dim)]) for _ in range(depth)])

    def forward(self, x):
        for attn, ff in self.layers:
            x = attn(x) + x
            x = ff(x) + x
        return x


def block_pair(B, T, dim, heads, dh, W, depth):
    """(restated reference in fp32 with the parameter initialisation of test_local_transformer_vs_restated_library, ours on the GPU)"""
    S = _mods()
    torch.manual_seed(B * 1000 + T)
    ref = RefLocalTransformer(dim, heads, dh, W, depth)
    for n, p in ref.named_parameters():                             # non-trivial norms / scales / gates
        with torch.no_grad():
            if p.dim() == 1:
                p.copy_(1.0 + 0.3 * torch.randn_like(p) if ('scale' in n or n.endswith('weight')) else 0.2 * torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) * p.shape[1] ** -0.5)
    ours = S.LocalTransformer(dim=dim, depth=depth, heads=heads, window_size=W, dim_head=dh, prenorm=True, causal=True)
    missing, unexpected = ours.load_state_dict(ref.state_dict(), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return ref, ours.to(dev())


def block_ref_grads(ref, x, gy, dtype=F64):
    ref = ref.to(dtype)
    ref.zero_grad(set_to_none=True)
    x64 = x.detach().clone().to(dtype).requires_grad_()
    ref(x64).backward(gy.to(dtype))
    return x64.grad, {k: p.grad for k, p in ref.named_parameters()}


def block_run(ours, x, gy):
    ours.train().zero_grad(set_to_none=True)
    xd = x.to(dev()).requires_grad_()
    y = ours(xd)
    assert y.grad_fn is not None
    y.backward(gy.to(dev()))
    return y.detach(), xd.grad, {k: p.grad for k, p in ours.named_parameters()}


BLOCK_SHAPES = [(2, 300, 512, 8, 64, 128, 1), (1, 129, 64, 2, 32, 64, 2), (2, 40, 64, 2, 32, 64, 1), (2, 50, 32, 2, 32, 16, 1), (1, 64, 48, 3, 32, 64, 1)]


@pytest.mark.parametrize('B,T,dim,heads,dh,W,depth', BLOCK_SHAPES)
def test_local_transformer_backward(B, T, dim, heads, dh, W, depth):
    ref, ours = block_pair(B, T, dim, heads, dh, W, depth)
    x, gy = rnd(B, T, dim, seed=T), rnd(B, T, dim, seed=T + 1)
    rdx, rgrads = block_ref_grads(ref, x, gy)
    with torch.no_grad():
        y_eval = ours.eval()(x.to(dev()))
    assert y_eval.grad_fn is None and ours(x.to(dev()).requires_grad_()).grad_fn is None           # eval mode: no graph, grad mode on or off
    y, dx, grads = block_run(ours, x, gy)
    with torch.no_grad():
        assert ours(x.to(dev())).grad_fn is None                                                     # training mode under no_grad: no graph
    assert torch.equal(y, y_eval), 'training-mode output differs from the eval-mode output'
    check('dx', dx, rdx)
    assert set(grads) == set(rgrads)
    for k, r in rgrads.items():
        check(k, grads[k], r)
    y2, dx2, grads2 = block_run(ours, x, gy)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_frozen_parameter_gets_no_gradient():
    B, T, dim, heads, dh, W, depth = 1, 129, 64, 2, 32, 64, 2
    _, ours = block_pair(B, T, dim, heads, dh, W, depth)
    x, gy = rnd(B, T, dim, seed=T), rnd(B, T, dim, seed=T + 1)
    _, dx, grads = block_run(ours, x, gy)
    frozen = 'layers.0.0.to_qkv.weight'
    dict(ours.named_parameters())[frozen].requires_grad_(False)
    _, dx2, grads2 = block_run(ours, x, gy)
    assert grads2[frozen] is None
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads if k != frozen)


def test_local_mha_forward_is_differentiable():
    """LocalMHA.forward, the (b, n, c) entry point without the residual, against float64 autograd of the restated LocalMHA"""
    B, T, dim, heads, dh, W = 2, 50, 32, 2, 32, 16
    ref, ours = block_pair(B, T, dim, heads, dh, W, 1)
    x, gy = rnd(B, T, dim, seed=7), rnd(B, T, dim, seed=8)
    mha64 = ref.layers[0][0].double()
    x64 = x.double().requires_grad_()
    mha64(x64).backward(gy.double())
    mha = ours.layers[0][0].train()
    xd = x.to(dev()).requires_grad_()
    mha(xd).backward(gy.to(dev()))
    check('dx', xd.grad, x64.grad)
    for k, p in mha64.named_parameters():
        check(k, dict(mha.named_parameters())[k].grad, p.grad)


# ---------------------------------------------------------------------------------------------- 4. end to end against the real reference

STACKS = ('encoder.', 'encoder_attn.', 'decoder_attn.', 'decoder.')


@pytest.fixture(scope='module')
def golden():
    fx = torch.load(os.path.join(GOLDEN_DIR, 'codec_bwd_local_attn_small.pt'), weights_only=False)
    return fx


def _codec(fx):
    S = _mods()
    ss = S.SoundStream(**fx['ctor'])
    assert ss.encoder_attn is not None and ss.decoder_attn is not None
    sd = synth_state_dict(fx['shapes'], fx['seed'])
    own = ss.state_dict()
    for k in fx['const_keys']:
        sd[k] = own[k].clone()                                      # rotary inv_freq: a constant buffer on both sides
    missing, unexpected = ss.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(STACKS)]
    return ss.to(dev()), sd


def _wave(fx):
    wave = fx['inputs']['wave'].float()
    return wave[:, None, :wave.shape[-1] // 320 * 320].contiguous()


def test_default_soundstream_gradients_match_the_reference(golden):
    fx = golden
    ss, _ = _codec(fx)
    x = _wave(fx).to(dev())
    with torch.no_grad():
        y_eval = ss.decode(ss.encode(x))                                 # eval mode (the constructor ends in eval())
    assert y_eval.grad_fn is None and ss.decode(ss.encode(x)).grad_fn is None
    ss.train()
    runs = []
    for _ in range(2):
        ss.zero_grad(set_to_none=True)
        y = ss.decode(ss.encode(x))
        assert y.grad_fn is not None
        loss = F.mse_loss(y, x)
        loss.backward()
        runs.append({k: p.grad.clone() for k, p in ss.named_parameters() if k.startswith(STACKS)})
    assert torch.equal(y.detach(), y_eval), 'training-mode output differs from the eval-mode output'
    ref = fx['outputs']
    e = abs(float(loss.detach()) - float(ref['loss'])) / abs(float(ref['loss']))
    print(f'loss rel {e:.3e}')
    assert e <= 1e-5
    assert set(runs[0]) == set(ref['grads'])
    print('worst gradient rel-max', max((relmax(runs[0][k], gr), k) for k, gr in ref['grads'].items()))
    for k, gr in ref['grads'].items():
        check(k, runs[0][k], gr)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


# ---------------------------------------------------------------------------------------------- 5. weight-image invalidation

def _restated_codec_loss(p64, x64, fx):
    """float64 restatement of decode(encode(x)) for the default constructor: the oracle's conv stacks around the restated LocalTransformer"""
    import audiolm_oracle as O
    c = fx['ctor']
    strides = tuple(c['strides'])

    def attn_stack(prefix, h):
        lt = RefLocalTransformer(c['codebook_dim'], c['attn_heads'], c['attn_dim_head'], c['attn_window_size'], c['attn_depth']).double()
        sub = {k[len(prefix):]: v for k, v in p64.items() if k.startswith(prefix)}
        assert set(sub) == set(lt.state_dict())
        return torch.func.functional_call(lt, sub, (h,))
    h = O.soundstream_encoder(p64, x64, strides=strides).transpose(1, 2)                             # 'b c n -> b n c'
    h = attn_stack('decoder_attn.', attn_stack('encoder_attn.', h))
    return F.mse_loss(O.soundstream_decoder(p64, h.transpose(1, 2), strides=strides), x64)


def test_two_sgd_steps_pick_up_in_place_updates(golden):
    """an in-place optimiser step must invalidate the forward AND the transposed weight images of the conv stacks and of the LocalTransformer's
    Linear layers: the later losses follow the float64 restatement's"""
    fx = golden
    ss, sd = _codec(fx)
    ss.train()
    x = _wave(fx)
    names = [k for k in sd if k.startswith(STACKS) and k not in fx['const_keys']]
    consts = {k: ss.state_dict()[k].double().cpu() for k in fx['const_keys']}
    lr = 1e-4
    ref = {k: sd[k].double().clone() for k in names}
    ref_losses, losses = [], []
    xd = x.to(dev())
    params = dict(ss.named_parameters())
    assert set(names) == {k for k in params if k.startswith(STACKS)}
    for step in range(3):
        p64 = {k: v.clone().requires_grad_() for k, v in ref.items()}
        l64 = _restated_codec_loss({**p64, **consts}, x.double(), fx)
        l64.backward()
        ref_losses.append(float(l64.detach()))
        ref = {k: (v - lr * p64[k].grad).detach() for k, v in ref.items()}
        ss.zero_grad(set_to_none=True)
        loss = F.mse_loss(ss.decode(ss.encode(xd)), xd)
        losses.append(float(loss.detach()))
        if step < 2:
            loss.backward()
            with torch.no_grad():
                for k in names:
                    params[k].add_(params[k].grad, alpha=-lr)
    print('losses', losses, 'restatement', ref_losses)
    assert abs(ref_losses[1] - ref_losses[0]) > 1e-4 * ref_losses[0]      # the step moves the loss by far more than the bound below
    for got, want in zip(losses, ref_losses):
        assert abs(got - want) <= 1e-5 * abs(want), (losses, ref_losses)


def test_unsupported_geometry_still_raises_before_any_launch(monkeypatch):
    S = _mods()
    from audiolm_pytorch_amd import _lib
    ss = S.SoundStream(channels=4, codebook_dim=16, codebook_size=32, rq_num_quantizers=4, attn_window_size=8, attn_dim_head=8, attn_heads=2).to(dev()).train()
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(NotImplementedError, match='LocalTransformer backward.*32 and 64'):
        ss.encode(rnd(1, 1, 640, seed=50).to(dev()))
    with pytest.raises(NotImplementedError, match='LocalTransformer backward.*32 and 64'):
        ss.decode(torch.zeros(1, 2, 16, device=dev()))
    assert not calls, calls
