"""The residual finite scalar quantizer on the MI355X (csrc/fsq.hip, codec_bwd.FsqFn, soundstream.GroupedResidualFSQ,
SoundStream(use_finite_scalar_quantizer=True)) against the float64 restatement tests/fsq_restated.py and its torch autograd.

Measure: the project's rel-max (max |a - b| / max |b|) with TOL = 2e-5 (tests/test_gpu_codec_bwd.py); every case runs twice and must be bitwise equal.

Index equality.  A device tanhf one ulp off can flip the rounding at a tie, and a flip changes the rest of that token's chain.  A token is NEAR A TIE
if, in the oracle, some |b_q[j] - floor(b_q[j]) - 0.5| < BAND = 1e-4 at an active layer.  The small cases use seeds, chosen on the CPU, for which the
oracle has no such token (asserted, with the margin that was seen when they were chosen), so every index must be equal; the large forward leaves
the near-tie tokens out of the idx / out comparison, asserts that they are at most 2 % of the tokens (the oracle alone: at most 0.6 % for
z ~ N(0, 1.5^2), Q up to 8), and checks every token, left out or not, for indices in range and decode(idx) = out within TOL.

Measured on the MI355X: worst rel-max over this file 3.2e-7 (a db_in); the large forward has 0.24 % of its tokens inside the band and no index that
differs from the oracle, inside the band or outside (which also says why the kernels carry z and the chain in double: in fp32 the
indices of the deep layers are rounding noise).
"""
import functools

import pytest
import torch

import fsq_restated as R

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
BAND = 1e-4
Z_STD = 1.5


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import ops
    return ops


@pytest.fixture(scope='module')
def S():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import soundstream
    return soundstream


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def check(name, got, want, tol=TOL):
    err = relmax(got, want)
    print(f'{name}: rel-max {err:.3e}')
    assert err <= tol, (name, err)


def tie_distance(bs):
    """smallest |b - floor(b) - 0.5| over the active layers"""
    return float((bs - torch.floor(bs) - 0.5).abs().min())


# ---------------------------------------------------------------------------------------------- kernel level

# (M, dim_g, levels, Q, k, seed): the seed is one for which the oracle has no near-tie token.  The last case is not a multiple of four wide: the
# kernels' scalar-access path.
KERNEL_CASES = [
    (197, 24, (4, 3), 3, 2, 1),
    (1, 512, (8, 5, 5, 5), 8, 7, 0),
    (300, 512, (8, 5, 5, 5), 8, 4, 1),
    (257, 1024, (8, 8, 8, 5, 5, 5), 4, 3, 8),
    (130, 4, (8, 5, 5, 5), 2, 1, 2),
    (45, 30, (8, 5, 5, 5), 3, 2, 0),
    (67, 40, (4, 3, 3, 3, 3, 2, 2, 2), 2, 1, 5),       # d = 8: the LDS row stride equals d
    (50, 36, (5, 5, 5, 4, 4, 3, 3), 3, 2, 0),          # d = 7
    (33, 258, (8, 5, 5, 5), 3, 2, 0),                  # scalar accesses, two column passes, a ragged last piece
]


def kernel_inputs(M, dim_g, levels, Q, k, seed):
    """fp32 inputs on the CPU: x and g as (M, 2 dim_g) matrices whose SECOND column half is the group under test, weights giving z of order 1.5"""
    g = torch.Generator().manual_seed(1000 + seed)
    d = len(levels)
    x = torch.randn(M, 2 * dim_g, generator=g)
    gout = torch.randn(M, 2 * dim_g, generator=g)
    if dim_g == d:
        x = x * Z_STD
        weights = None
    else:
        weights = (torch.randn(d, dim_g, generator=g) * (Z_STD / dim_g ** 0.5), torch.randn(d, generator=g) * 0.1,
                   torch.randn(dim_g, d, generator=g) * 0.5, torch.randn(dim_g, generator=g) * 0.1)
    return x, gout, weights


@functools.lru_cache(maxsize=None)
def kernel_reference(M, dim_g, levels, Q, k, seed):
    """float64 oracle of one case, computed once: out, idx, z, input and parameter gradients for the case's g, decode(idx), the tie distance"""
    x, gout, weights = kernel_inputs(M, dim_g, levels, Q, k, seed)
    xs = x[:, dim_g:].to(F64).requires_grad_()
    ws = None if weights is None else tuple(w.to(F64).requires_grad_() for w in weights)
    grp = R.GroupFSQ(list(levels), Q, ws)
    out, idx, z, _, bs = grp.forward(xs, k)
    (out * gout[:, dim_g:].to(F64)).sum().backward()
    with torch.no_grad():
        dec = grp.decode(idx)
    grads = () if ws is None else tuple(w.grad for w in ws)
    return dict(out=out.detach(), idx=idx, z=z.detach(), dx=xs.grad, grads=grads, dec=dec, tie=tie_distance(bs), z_std=float(z.detach().std()))


def run_kernels(ops, M, dim_g, levels, Q, k, seed):
    x, gout, weights = kernel_inputs(M, dim_g, levels, Q, k, seed)
    d = len(levels)
    xd, gd = x.to(dev()), gout.to(dev())
    wd = None if weights is None else tuple(w.to(dev()) for w in weights)
    consts = ops.fsq_constants(levels, Q).to(dev())
    out = torch.full((M, 2 * dim_g), 7., device=dev())
    dx = torch.full((M, 2 * dim_g), 7., device=dev())
    dec = torch.full((M, 2 * dim_g), 7., device=dev())
    idx = torch.full((M, 2 * Q), -7, dtype=torch.int64, device=dev())
    z = ops.fsq_fwd(xd[:, dim_g:], wd, consts, d, Q, k, idx[:, Q:], out[:, dim_g:], save_z=wd is not None)
    grads = ops.fsq_bwd(gd[:, dim_g:], xd[:, dim_g:], z, wd, consts, d, Q, k, dx[:, dim_g:])
    ops.fsq_decode(idx[:, Q:], wd, consts, d, Q, dec[:, dim_g:])
    torch.cuda.synchronize()
    for full in (out, dx, dec):                                  # the other group's columns are not touched: the leading dimensions are honoured
        assert bool((full[:, :dim_g] == 7.).all())
    assert bool((idx[:, :Q] == -7).all())
    return dict(out=out[:, dim_g:].clone(), idx=idx[:, Q:].clone(), z=z, dx=dx[:, dim_g:].clone(), grads=grads, dec=dec[:, dim_g:].clone())


@pytest.mark.parametrize('M,dim_g,levels,Q,k,seed', KERNEL_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_kernels_forward_backward_decode(ops, M, dim_g, levels, Q, k, seed):
    ref = kernel_reference(M, dim_g, levels, Q, k, seed)
    print(f'oracle: tie distance {ref["tie"]:.3e}, z std {ref["z_std"]:.3f}')
    assert ref['tie'] >= BAND, 'the seed must give the oracle no near-tie token'
    assert 0.75 <= ref['z_std'] <= 3.0 or M == 1, 'z must be of order 1.5: a chain in tanh saturation tests nothing'
    a, b = (run_kernels(ops, M, dim_g, levels, Q, k, seed) for _ in range(2))
    for key in ('out', 'idx', 'dx', 'dec'):
        assert torch.equal(a[key], b[key]), key
    assert all(torch.equal(u, v) for u, v in zip(a['grads'], b['grads'])) and len(a['grads']) == (0 if dim_g == len(levels) else 4)
    assert torch.equal(a['idx'].cpu(), ref['idx'])
    assert bool((ref['idx'][:, k + 1:] == -1).all()) and bool((ref['idx'][:, :k + 1] >= 0).all())
    check('out', a['out'], ref['out'])
    check('dx', a['dx'], ref['dx'])
    check('decode vs oracle', a['dec'], ref['dec'])
    check('decode vs forward', a['dec'], a['out'])
    if a['z'] is not None:
        assert torch.equal(a['z'], b['z'])
        check('z', a['z'], ref['z'])
    for name, got, want in zip(('dW_in', 'db_in', 'dW_out', 'db_out'), a['grads'], ref['grads']):
        check(name, got, want)


def test_kernel_limits_are_refused(ops):
    from audiolm_pytorch_amd import _lib
    x = torch.zeros(4, 2048, device=dev())
    consts = ops.fsq_constants((4, 3), 2).to(dev())
    w = (torch.zeros(2, 2048, device=dev()), torch.zeros(2, device=dev()), torch.zeros(2048, 2, device=dev()), torch.zeros(2048, device=dev()))
    with pytest.raises(_lib.AlmError, match='ALM_ERR_UNSUPPORTED'):
        ops.fsq_fwd(x, w, consts, 2, 2, 1, torch.zeros(4, 2, dtype=torch.int64, device=dev()), torch.empty_like(x))
    assert _lib.query('alm_fsq_bwd_ws_floats', 4, 2048, 2) == -1 and _lib.query('alm_fsq_bwd_ws_floats', 130, 4, 4) == 0
    assert _lib.query('alm_fsq_consts_floats', 33) == -1 and _lib.query('alm_fsq_consts_floats', 8) == 56 + 128


# ---------------------------------------------------------------------------------------------- one larger forward

def test_large_forward_outside_the_tie_band(ops):
    M, dim_g, levels, Q = 4096, 512, (8, 5, 5, 5), 8
    d = len(levels)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, dim_g, generator=g)
    weights = (torch.randn(d, dim_g, generator=g) * (Z_STD / dim_g ** 0.5), torch.randn(d, generator=g) * 0.1,
               torch.randn(dim_g, d, generator=g) * 0.5, torch.randn(dim_g, generator=g) * 0.1)
    grp = R.GroupFSQ(list(levels), Q, tuple(w.to(F64) for w in weights))
    ref_out, ref_idx, _, _, bs = grp.forward(x.to(F64))
    near = R.near_tie(bs, BAND)
    share = float(near.double().mean())
    print(f'near-tie share {share:.4%} of {M} tokens')
    assert share <= 0.02
    keep = ~near
    xd, wd, consts = x.to(dev()), tuple(w.to(dev()) for w in weights), ops.fsq_constants(levels, Q).to(dev())
    runs = []
    for _ in range(2):
        out, idx, dec = torch.empty(M, dim_g, device=dev()), torch.empty(M, Q, dtype=torch.int64, device=dev()), torch.empty(M, dim_g, device=dev())
        ops.fsq_fwd(xd, wd, consts, d, Q, Q - 1, idx, out)
        ops.fsq_decode(idx, wd, consts, d, Q, dec)
        runs.append((out, idx, dec))
    (out, idx, dec), (out2, idx2, dec2) = runs
    assert torch.equal(out, out2) and torch.equal(idx, idx2) and torch.equal(dec, dec2)
    assert int(idx.min()) >= 0 and int(idx.max()) < 1000        # every token, left out or not
    check('decode(idx) vs out, all tokens', dec, out)
    flipped = int((idx.cpu() != ref_idx).any(dim=-1).sum())
    print(f'tokens with an index that differs from the oracle: {flipped} (all inside the band)')
    assert torch.equal(idx.cpu()[keep], ref_idx[keep])
    check('out outside the band', out.cpu()[keep], ref_out[keep])


# ---------------------------------------------------------------------------------------------- module level, groups = 2

MOD_KW = dict(dim=64, levels=[8, 5, 5, 5], num_quantizers=4, groups=2)
MOD_SEED = 1


def _module(S):
    torch.manual_seed(4321 + MOD_SEED)
    rq = S.GroupedResidualFSQ(**MOD_KW)
    x = torch.randn(2, 37, 64, generator=torch.Generator().manual_seed(99 + MOD_SEED)) * 2.6       # default nn.Linear init: z std = x std / sqrt(3)
    gout = torch.randn(2, 37, 64, generator=torch.Generator().manual_seed(98))
    return rq, x, gout


@functools.lru_cache(maxsize=None)
def _module_reference(k):
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import soundstream
    rq, x, gout = _module(soundstream)
    oracle = R.GroupedFSQ.from_module(rq, F64, requires_grad=True)
    xs = x.to(F64).requires_grad_()
    out, idx, bss = oracle.forward(xs, k)
    (out * gout.to(F64)).sum().backward()
    grads = [p.grad for grp in oracle.groups for p in grp.weights]
    return dict(out=out.detach(), idx=idx, dx=xs.grad, grads=grads, tie=min(tie_distance(bs) for bs in bss))


def test_module_training_forward_and_gradients(S):
    k = 2
    ref = _module_reference(k)
    assert ref['tie'] >= BAND
    runs = []
    for _ in range(2):
        rq, x, gout = _module(S)
        rq = rq.to(dev()).train()
        rq.dropout_index = lambda: k
        xd = x.to(dev()).requires_grad_()
        out, idx = rq(xd)
        assert out.requires_grad and not idx.requires_grad and idx.dtype == torch.int64 and idx.shape == (2, 2, 37, 4)
        (out * gout.to(dev())).sum().backward()
        runs.append((out.detach(), idx, xd.grad, [p.grad for p in rq.parameters()]))
    (out, idx, dx, grads), (out2, idx2, dx2, grads2) = runs
    assert torch.equal(out, out2) and torch.equal(idx, idx2) and torch.equal(dx, dx2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert torch.equal(idx.cpu(), ref['idx']) and bool((idx[..., k + 1:] == -1).all())
    check('out', out, ref['out'])
    check('x.grad', dx, ref['dx'])
    names = [n for n, _ in S.GroupedResidualFSQ(**MOD_KW).named_parameters()]
    assert len(grads) == len(ref['grads']) == len(names) == 8
    for name, got, want in zip(names, grads, ref['grads']):
        check(name, got, want)


def test_module_eval_uses_all_layers_and_records_nothing(S):
    ref = _module_reference(3)
    assert ref['tie'] >= BAND
    rq, x, _ = _module(S)
    rq = rq.to(dev()).eval()
    rq.dropout_index = lambda: 0                                 # must not be consulted in eval mode
    xd = x.to(dev()).requires_grad_()
    out, idx = rq(xd)
    out2, idx2 = rq(xd)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out, out2) and torch.equal(idx, idx2)
    assert torch.equal(idx.cpu(), ref['idx']) and int(idx.min()) >= 0
    check('out', out, ref['out'])
    # fewer than Q columns, and -1 entries
    oracle = R.GroupedFSQ.from_module(rq, F64)
    check('decode, all columns', rq.get_output_from_indices(idx), out)
    part = idx[..., :2].contiguous()
    check('decode, 2 of 4 columns', rq.get_output_from_indices(part), oracle.decode(part.cpu()))
    holes = idx.clone()
    holes[:, :, ::3, 1] = -1
    holes[:, 1, :, 3] = -1
    got = rq.get_output_from_indices(holes)
    check('decode with -1 entries', got, oracle.decode(holes.cpu()))
    assert torch.equal(got, rq.get_output_from_indices(holes)) and not torch.equal(got, out)


def test_module_identity_projection_training(S):
    """dim / groups == len(levels): no parameters, the graph runs from the input alone"""
    rq = S.GroupedResidualFSQ(dim=8, levels=[8, 5, 5, 5], num_quantizers=2, groups=2).to(dev()).train()
    rq.dropout_index = lambda: 1
    g = torch.Generator().manual_seed(13)
    x, gout = torch.randn(3, 50, 8, generator=g) * Z_STD, torch.randn(3, 50, 8, generator=g)
    oracle = R.GroupedFSQ.from_module(rq, F64)
    xs = x.to(F64).requires_grad_()
    ref_out, ref_idx, bss = oracle.forward(xs, 1)
    (ref_out * gout.to(F64)).sum().backward()
    assert min(tie_distance(bs) for bs in bss) >= BAND
    xd = x.to(dev()).requires_grad_()
    out, idx = rq(xd)
    (out * gout.to(dev())).sum().backward()
    assert torch.equal(idx.cpu(), ref_idx)
    check('out', out, ref_out)
    check('x.grad', xd.grad, xs.grad)
    with torch.no_grad():
        assert not rq(xd)[0].requires_grad


# ---------------------------------------------------------------------------------------------- SoundStream end to end

SS_KW = dict(channels=4, strides=(2, 4, 5, 8), codebook_dim=16, rq_num_quantizers=3, use_local_attn=False, use_finite_scalar_quantizer=True,
             finite_scalar_quantizer_levels=[4, 3])


def _soundstream(S, **kw):
    torch.manual_seed(1234)
    ss = S.SoundStream(**SS_KW, **kw).to(dev())
    x = torch.randn(2, 320 * 12, generator=torch.Generator().manual_seed(77)) * 0.5
    return ss, x.to(dev())


def test_soundstream_codec_paths(S):
    ss, x = _soundstream(S)
    assert not ss.training and ss.codebook_size == 12
    quantized, indices, commit = ss(x, return_encoded=True)
    feats = ss.encode(ss.process_input(x)[0])
    q2, i2 = ss.rq(feats)
    b, n = feats.shape[:2]
    assert n == 12 and torch.equal(quantized, q2) and torch.equal(indices, i2.permute(1, 2, 0, 3).reshape(b, n, -1))     # 'g b n q -> b n (g q)'
    assert commit.ndim == 0 and float(commit) == 0. and not quantized.requires_grad
    codes = ss(x, return_codes_only=True)
    assert torch.equal(codes, i2) and torch.equal(ss.tokenize(x), i2) and int(codes.min()) >= 0 and int(codes.max()) < 12
    recon = ss(x, return_recons_only=True)
    assert recon.shape == (2, 1, 320 * 12)
    check('decode_from_codebook_indices (g b n q)', ss.decode_from_codebook_indices(codes), recon)
    check('decode_from_codebook_indices (b n (g q))', ss.decode_from_codebook_indices(indices), recon)
    check('decode(quantize=True)', ss.decode(feats, quantize=True), recon)


def test_soundstream_training_backward_is_finite_and_reproducible(S):
    ss, x = _soundstream(S)
    ss.train()
    ss.rq.dropout_index = lambda: 1
    grads = []
    for _ in range(2):
        ss.zero_grad(set_to_none=True)
        recon = ss(x, return_recons_only=True)
        assert recon.requires_grad
        recon.square().mean().backward()
        grads.append((ss.encoder[0].conv.weight.grad.clone(), ss.rq.rvqs[0].project_in.weight.grad.clone()))
    for a, b in zip(*grads):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)


def test_soundstream_loss_breakdown_has_zero_commitment(S):
    ss, x = _soundstream(S, with_discriminators=True, stft_discriminator=False, multi_spectral_recon_loss_weight=0)
    ss.train()
    total, (recon, multi_spectral, adversarial, feature, commitment) = ss(x, return_loss_breakdown=True)
    assert float(commitment) == 0. and float(multi_spectral) == 0. and float(recon) > 0 and bool(torch.isfinite(total))
    total.backward()
    assert float(ss.rq.rvqs[0].project_in.weight.grad.abs().max()) > 0                 # the generator loss reaches the quantizer's parameters
