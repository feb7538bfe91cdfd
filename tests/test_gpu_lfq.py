"""The residual lookup-free quantizer on the MI355X (csrc/lfq.hip, codec_bwd.LfqFn, soundstream.GroupedResidualLFQ,
SoundStream(use_lookup_free_quantizer=True, with_lfq=True)) against the float64 restatement tests/lfq_restated.py (the DENSE formulation: explicit
codebook, einsum, softmax, clamped log) and its torch autograd.

Measure: the project's rel-max (max |a - b| / max |b|) with TOL = 2e-5 (tests/test_gpu_fsq.py); every case runs twice and must be bitwise equal.

Index equality is unconditional: a bit is the sign of a residual, the kernels carry z and the chain in double, and the seeds are ones, chosen on the
CPU, for which the oracle's smallest |r_q| over the active layers exceeds MARGIN = 1e-7 (asserted), ten orders above the rounding of a float64 dot
product.  No token is left out.

The backward is checked three times -- g_out alone, g_loss alone, both -- because the loss part of dz is about 1 % of (k + 1) g_z and a rel-max over
the sum would hide it.

One reference is identically zero: with ONE token, gamma = 1 and no commitment term, H(p) - gamma H(mean p) = 0, so those losses and their gradient
are a difference of two equal terms and max |b| is 0 (or rounding noise).  There, and only there, the denominator is the first of the two cancelling
terms (the oracle run once more with gamma = 0): the error is still measured against the precision the terms are computed to, with the same TOL.

Measured on the MI355X: worst rel-max over this file 3.8e-7 (a db_in); the one-token case against its cancelling term 4e-18 (losses) and 3.5e-16
(gradients); every index equal to the oracle's (which also says why the kernels carry z, the chain and the softmax in double).
"""
import functools

import pytest
import torch

import lfq_restated as R

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5
MARGIN = 1e-7
Z_STD = 1.5
W_E, GAMMA = 0.1, 1.


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


def relmax(a, b, floor=0.):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=max(floor, 1e-30)))


def check(name, got, want, floor=0.):
    err = relmax(got, want, floor)
    print(f'{name}: rel-max {err:.3e}' + (f' (against the cancelling term {floor:.3e})' if floor else ''))
    assert err <= TOL, (name, err)


def smallest_residual(rs):
    return float(rs.abs().min())


# ---------------------------------------------------------------------------------------------- kernel level

# (M, dim_g, codebook_size, Q, k, seed): the seed is one for which the oracle's smallest |r_q| exceeds MARGIN.  In order: plain; the mean over one
# token; quantize dropout; the identity projection; the scalar-access path (30 is no multiple of 4); d = 1; four reduction chunks of the code
# distribution (three of 64 rows and a ragged one of 17) at 1024 codes
KERNEL_CASES = [
    (197, 24, 32, 3, 2, 0),
    (1, 512, 1024, 8, 7, 0),
    (300, 512, 1024, 8, 4, 0),
    (130, 4, 16, 2, 1, 0),
    (45, 30, 256, 3, 2, 0),
    (257, 128, 2, 2, 1, 0),
    (209, 64, 1024, 8, 7, 0),
    (67, 40, 128, 2, 1, 0),                            # d = 7
    (50, 36, 512, 3, 2, 0),                            # d = 9
    (41, 20, 8, 2, 1, 0),                              # d = 3
    (33, 258, 64, 3, 2, 0),                            # d = 6, scalar accesses, two column passes
]
COMMIT_WEIGHTS = (0., 0.25)
MODES = ('g_out', 'g_loss', 'both')


def kernel_inputs(M, dim_g, codebook_size, Q, k, seed):
    """fp32 inputs on the CPU: x and g as (M, 2 dim_g) matrices whose SECOND column half is the group under test, weights giving z ~ N(0, 1.5^2)
    (layer 0 is then deep in the softmax's saturation and the deep layers far from it), and the per-layer loss gradients"""
    g = torch.Generator().manual_seed(2000 + seed)
    d = codebook_size.bit_length() - 1
    x = torch.randn(M, 2 * dim_g, generator=g)
    gout = torch.randn(M, 2 * dim_g, generator=g)
    gloss = torch.randn(Q, generator=g)
    if dim_g == d:
        x = x * Z_STD
        weights = None
    else:
        weights = (torch.randn(d, dim_g, generator=g) * (Z_STD / dim_g ** 0.5), torch.randn(d, generator=g) * 0.1,
                   torch.randn(dim_g, d, generator=g) * 0.5, torch.randn(dim_g, generator=g) * 0.1)
    return x, gout, gloss, weights


def _oracle_run(case, w_c, gamma):
    M, dim_g, codebook_size, Q, k, seed = case
    x, gout, gloss, weights = kernel_inputs(*case)
    xs = x[:, dim_g:].to(F64).requires_grad_()
    ws = None if weights is None else tuple(w.to(F64).requires_grad_() for w in weights)
    grp = R.GroupLFQ(codebook_size, Q, ws, (R.INV_TEMPERATURE, W_E, w_c, gamma))
    out, idx, losses, z, _, rs = grp.forward(xs, k)
    leaves = (xs,) + (ws or ())
    heads = dict(g_out=(out * gout[:, dim_g:].to(F64)).sum(), g_loss=(losses * gloss.to(F64)).sum())
    heads['both'] = heads['g_out'] + heads['g_loss']
    grads = {}
    for mode in MODES:
        gs = torch.autograd.grad(heads[mode], leaves, retain_graph=True, allow_unused=True)
        grads[mode] = [torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)]
    with torch.no_grad():
        dec = grp.decode(idx)
    return dict(out=out.detach(), idx=idx, z=z.detach(), losses=losses.detach(), grads=grads, dec=dec, margin=smallest_residual(rs),
                z_std=float(z.detach().std()) if M > 1 else 0.)


@functools.lru_cache(maxsize=None)
def kernel_reference(case, w_c):
    """float64 oracle of one case and one commitment weight, computed once.  `floors`: for the one-token case without a commitment term, the
    magnitudes of the first cancelling term (gamma = 0) of the losses and of the g_loss-alone gradients; else empty"""
    ref = _oracle_run(case, w_c, GAMMA)
    ref['floors'] = {}
    if case[0] == 1 and w_c == 0:
        first = _oracle_run(case, w_c, 0.)
        ref['floors'] = dict(losses=float(first['losses'].abs().max()), grads=[float(g.abs().max()) for g in first['grads']['g_loss']])
    return ref


def run_kernels(ops, case, w_c):
    M, dim_g, codebook_size, Q, k, seed = case
    x, gout, gloss, weights = kernel_inputs(*case)
    d = codebook_size.bit_length() - 1
    cfg = (R.INV_TEMPERATURE, W_E, w_c, GAMMA)
    xd, gd, gl = x.to(dev()), gout.to(dev()), gloss.to(dev())
    wd = None if weights is None else tuple(w.to(dev()) for w in weights)
    out = torch.full((M, 2 * dim_g), 7., device=dev())
    dec = torch.full((M, 2 * dim_g), 7., device=dev())
    idx = torch.full((M, 2 * Q), -7, dtype=torch.int64, device=dev())
    z, losses, avg = ops.lfq_fwd(xd[:, dim_g:], wd, d, Q, k, idx[:, Q:], out[:, dim_g:], loss_cfg=cfg)
    ops.lfq_decode(idx[:, Q:], wd, d, Q, dec[:, dim_g:])
    res = dict(z=z, losses=losses, avg=avg, grads={})
    zero_g = torch.zeros_like(gd)
    for mode in MODES:
        dx = torch.full((M, 2 * dim_g), 7., device=dev())
        g_in = zero_g if mode == 'g_loss' else gd
        grads = ops.lfq_bwd(g_in[:, dim_g:], None if mode == 'g_out' else gl, xd[:, dim_g:], z, avg, wd, d, Q, k, dx[:, dim_g:], cfg)
        assert bool((dx[:, :dim_g] == 7.).all())
        res['grads'][mode] = [dx[:, dim_g:].clone(), *grads]
    # eval-style call: no losses, the same indices and output
    out_e = torch.full((M, 2 * dim_g), 7., device=dev())
    idx_e = torch.full((M, 2 * Q), -7, dtype=torch.int64, device=dev())
    assert ops.lfq_fwd(xd[:, dim_g:], wd, d, Q, k, idx_e[:, Q:], out_e[:, dim_g:]) == (None, None, None)
    torch.cuda.synchronize()
    for full in (out, dec, out_e):                               # the other group's columns are not touched: the leading dimensions are honoured
        assert bool((full[:, :dim_g] == 7.).all())
    assert bool((idx[:, :Q] == -7).all()) and torch.equal(idx, idx_e) and torch.equal(out, out_e)
    res.update(out=out[:, dim_g:].clone(), idx=idx[:, Q:].clone(), dec=dec[:, dim_g:].clone())
    return res


@pytest.mark.parametrize('w_c', COMMIT_WEIGHTS)
@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_kernels_forward_backward_decode(ops, case, w_c):
    M, dim_g, codebook_size, Q, k, seed = case
    d = codebook_size.bit_length() - 1
    ref = kernel_reference(case, w_c)
    print(f'oracle: smallest |r_q| {ref["margin"]:.3e}, z std {ref["z_std"]:.3f}, losses {ref["losses"].tolist()}')
    assert ref['margin'] > MARGIN, 'the seed must keep every residual of the oracle away from zero'
    assert 0.75 <= ref['z_std'] <= 3.0 or M == 1, 'z must be of order 1.5'
    a, b = (run_kernels(ops, case, w_c) for _ in range(2))
    for key in ('out', 'idx', 'dec', 'z', 'losses', 'avg'):
        assert torch.equal(a[key], b[key]), key
    for mode in MODES:
        assert all(torch.equal(u, v) for u, v in zip(a['grads'][mode], b['grads'][mode])), mode
        assert len(a['grads'][mode]) == (1 if dim_g == d else 5)
    assert torch.equal(a['idx'].cpu(), ref['idx'])
    assert bool((ref['idx'][:, k + 1:] == -1).all()) and bool((ref['idx'][:, :k + 1] >= 0).all())
    check('out', a['out'], ref['out'])
    check('z', a['z'], ref['z'])
    check('decode vs oracle', a['dec'], ref['dec'])
    check('decode vs forward', a['dec'], a['out'])
    floors = ref['floors']
    check('losses', a['losses'], ref['losses'], floors.get('losses', 0.))
    assert bool((a['losses'][k + 1:] == 0).all())
    assert float((a['avg'][:k + 1].sum(dim=-1) - 1).abs().max()) <= 1e-12
    names = ('dx', 'dW_in', 'db_in', 'dW_out', 'db_out')
    for mode in MODES:
        for i, (name, got, want) in enumerate(zip(names, a['grads'][mode], ref['grads'][mode])):
            check(f'{mode}: {name}', got, want, floors['grads'][i] if floors and mode == 'g_loss' else 0.)
    if not floors:
        assert float(ref['grads']['g_loss'][0].abs().max()) > 0    # the loss gradient is there to be missed


def test_bad_arguments_are_refused_before_any_launch(ops):
    from audiolm_pytorch_amd import _lib
    M, dim_g, Q = 8, 16, 2
    x = torch.zeros(M, dim_g, device=dev())
    idx = torch.zeros(M, Q, dtype=torch.int64, device=dev())
    cfg = (R.INV_TEMPERATURE, W_E, 0., GAMMA)

    def weights(d, n=dim_g):
        return (torch.zeros(d, n, device=dev()), torch.zeros(d, device=dev()), torch.zeros(n, d, device=dev()), torch.zeros(n, device=dev()))
    with pytest.raises(_lib.AlmError, match='ALM_ERR_UNSUPPORTED'):                      # d above the limit
        ops.lfq_fwd(x, weights(11), 11, Q, 1, idx, torch.empty_like(x))
    with pytest.raises(_lib.AlmError, match='limits'):
        ops.lfq_fwd(x, weights(11), 11, Q, 1, idx, torch.empty_like(x), loss_cfg=cfg)
    wide = torch.zeros(M, 2048, device=dev())
    with pytest.raises(_lib.AlmError, match='ALM_ERR_UNSUPPORTED'):
        ops.lfq_fwd(wide, weights(4, 2048), 4, Q, 1, idx, torch.empty_like(wide))
    with pytest.raises(_lib.AlmError, match='ALM_ERR_BAD_ARG'):                          # a short workspace
        ops.lfq_fwd(x, weights(4), 4, Q, 1, idx, torch.empty_like(x), loss_cfg=cfg, ws=torch.zeros(8, dtype=F64, device=dev()))
    with pytest.raises(_lib.AlmError, match='ALM_ERR_BAD_ARG'):                          # k outside 0 .. Q - 1
        ops.lfq_fwd(x, weights(4), 4, Q, Q, idx, torch.empty_like(x))
    with pytest.raises(_lib.AlmError, match='expected'):                                 # a wrong dtype
        ops.lfq_fwd(x.double(), weights(4), 4, Q, 1, idx, torch.empty_like(x))
    with pytest.raises(_lib.AlmError, match='expected'):
        ops.lfq_fwd(x, weights(4), 4, Q, 1, idx.int(), torch.empty_like(x))
    z, losses, avg = ops.lfq_fwd(x, weights(4), 4, Q, 1, idx, torch.empty_like(x), loss_cfg=cfg)
    gl = torch.zeros(Q, device=dev())
    with pytest.raises(_lib.AlmError, match='ALM_ERR_BAD_ARG'):
        ops.lfq_bwd(x, gl, x, z, avg, weights(4), 4, Q, 1, torch.empty_like(x), cfg, ws=torch.zeros(8, device=dev()))
    with pytest.raises(_lib.AlmError, match='expected'):
        ops.lfq_bwd(x, gl, x, z.float(), avg, weights(4), 4, Q, 1, torch.empty_like(x), cfg)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- module level, groups = 2

MOD_KW = dict(dim=64, num_quantizers=4, codebook_size=32, groups=2, commitment_loss_weight=0.25)
MOD_SEED = 0


def _module(S):
    torch.manual_seed(4321 + MOD_SEED)
    rq = S.GroupedResidualLFQ(**MOD_KW)
    x = torch.randn(2, 37, 64, generator=torch.Generator().manual_seed(99 + MOD_SEED)) * 2.6       # default nn.Linear init: z std = x std / sqrt(3)
    gout = torch.randn(2, 37, 64, generator=torch.Generator().manual_seed(98))
    gloss = torch.randn(2, 4, generator=torch.Generator().manual_seed(97))
    return rq, x, gout, gloss


@functools.lru_cache(maxsize=None)
def _module_reference(k, train):
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import soundstream
    rq, x, gout, gloss = _module(soundstream)
    oracle = R.GroupedLFQ.from_module(rq, F64, requires_grad=True)
    xs = x.to(F64).requires_grad_()
    out, idx, losses, rss = oracle.forward(xs, k, train)
    ((out * gout.to(F64)).sum() + (losses * gloss.to(F64)).sum()).backward()
    grads = [p.grad for grp in oracle.groups for p in grp.weights]
    return dict(out=out.detach(), idx=idx, losses=losses.detach(), dx=xs.grad, grads=grads, margin=min(smallest_residual(rs) for rs in rss))


def test_module_training_forward_and_gradients(S):
    k = 2
    ref = _module_reference(k, True)
    assert ref['margin'] > MARGIN
    runs = []
    for _ in range(2):
        rq, x, gout, gloss = _module(S)
        rq = rq.to(dev()).train()
        rq.dropout_index = lambda: k
        xd = x.to(dev()).requires_grad_()
        out, idx, losses = rq(xd)
        assert out.requires_grad and losses.requires_grad and not idx.requires_grad and idx.dtype == torch.int64
        assert idx.shape == (2, 2, 37, 4) and losses.shape == (2, 4)
        ((out * gout.to(dev())).sum() + (losses * gloss.to(dev())).sum()).backward()
        runs.append((out.detach(), idx, losses.detach(), xd.grad, [p.grad for p in rq.parameters()]))
    (out, idx, losses, dx, grads), (out2, idx2, losses2, dx2, grads2) = runs
    assert torch.equal(out, out2) and torch.equal(idx, idx2) and torch.equal(losses, losses2) and torch.equal(dx, dx2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert torch.equal(idx.cpu(), ref['idx']) and bool((idx[..., k + 1:] == -1).all()) and bool((losses[:, k + 1:] == 0).all())
    check('out', out, ref['out'])
    check('losses', losses, ref['losses'])
    check('x.grad', dx, ref['dx'])
    names = [n for n, _ in S.GroupedResidualLFQ(**MOD_KW).named_parameters()]
    assert len(grads) == len(ref['grads']) == len(names) == 8
    for name, got, want in zip(names, grads, ref['grads']):
        check(name, got, want)


def test_module_eval_uses_all_layers_and_records_nothing(S):
    ref = _module_reference(3, False)
    assert ref['margin'] > MARGIN
    rq, x, _, _ = _module(S)
    rq = rq.to(dev()).eval()
    rq.dropout_index = lambda: 0                                 # must not be consulted in eval mode
    xd = x.to(dev()).requires_grad_()
    out, idx, losses = rq(xd)
    out2, idx2, _ = rq(xd)
    assert not out.requires_grad and out.grad_fn is None and not losses.requires_grad and torch.equal(out, out2) and torch.equal(idx, idx2)
    assert losses.shape == (2, 4) and bool((losses == 0).all())
    assert torch.equal(idx.cpu(), ref['idx']) and int(idx.min()) >= 0 and int(idx.max()) < 32
    check('out', out, ref['out'])
    # fewer than Q columns, and -1 entries
    oracle = R.GroupedLFQ.from_module(rq, F64)
    check('decode, all columns', rq.get_output_from_indices(idx), out)
    part = idx[..., :2].contiguous()
    check('decode, 2 of 4 columns', rq.get_output_from_indices(part), oracle.decode(part.cpu()))
    holes = idx.clone()
    holes[:, :, ::3, 1] = -1
    holes[:, 1, :, 3] = -1
    got = rq.get_output_from_indices(holes)
    check('decode with -1 entries', got, oracle.decode(holes.cpu()))
    assert torch.equal(got, rq.get_output_from_indices(holes)) and not torch.equal(got, out)


def test_module_no_grad_training_returns_losses_without_a_graph(S):
    k = 2
    ref = _module_reference(k, True)
    rq, x, _, _ = _module(S)
    rq = rq.to(dev()).train()
    rq.dropout_index = lambda: k
    with torch.no_grad():
        out, idx, losses = rq(x.to(dev()).requires_grad_())
    assert not out.requires_grad and not losses.requires_grad and out.grad_fn is None and losses.grad_fn is None
    assert torch.equal(idx.cpu(), ref['idx'])
    check('losses', losses, ref['losses'])
    assert float(losses[:, :k + 1].abs().min()) > 0


def test_module_identity_projection_training(S):
    """dim / groups == log2(codebook_size): no parameters, the graph runs from the input alone"""
    rq = S.GroupedResidualLFQ(dim=8, num_quantizers=2, codebook_size=16, groups=2).to(dev()).train()
    rq.dropout_index = lambda: 1
    g = torch.Generator().manual_seed(13)
    x, gout, gloss = torch.randn(3, 50, 8, generator=g) * Z_STD, torch.randn(3, 50, 8, generator=g), torch.randn(2, 2, generator=g)
    oracle = R.GroupedLFQ.from_module(rq, F64)
    xs = x.to(F64).requires_grad_()
    ref_out, ref_idx, ref_losses, rss = oracle.forward(xs, 1)
    assert min(smallest_residual(rs) for rs in rss) > MARGIN
    g_both, = torch.autograd.grad((ref_out * gout.to(F64)).sum() + (ref_losses * gloss.to(F64)).sum(), xs, retain_graph=True)
    g_loss, = torch.autograd.grad((ref_losses * gloss.to(F64)).sum(), xs)
    xd = x.to(dev()).requires_grad_()
    out, idx, losses = rq(xd)
    d_both, = torch.autograd.grad((out * gout.to(dev())).sum() + (losses * gloss.to(dev())).sum(), xd, retain_graph=True)
    d_loss, = torch.autograd.grad((losses * gloss.to(dev())).sum(), xd)
    assert torch.equal(idx.cpu(), ref_idx)
    check('out', out, ref_out)
    check('losses', losses, ref_losses)
    check('x.grad, both', d_both, g_both)
    check('x.grad, losses alone', d_loss, g_loss)
    with torch.no_grad():
        assert not rq(xd)[0].requires_grad


# ---------------------------------------------------------------------------------------------- SoundStream end to end

SS_KW = dict(channels=4, codebook_dim=16, rq_num_quantizers=3, codebook_size=32, use_lookup_free_quantizer=True, with_lfq=True, use_local_attn=False)


def _soundstream(S, **kw):
    torch.manual_seed(1234)
    ss = S.SoundStream(**SS_KW, **kw).to(dev())
    x = torch.randn(2, 320 * 12, generator=torch.Generator().manual_seed(77)) * 0.5
    return ss, x.to(dev())


def test_soundstream_codec_paths(S):
    ss, x = _soundstream(S)
    assert not ss.training and ss.codebook_size == 32 and ss.use_lookup_free_quantizer is True
    quantized, indices, commit = ss(x, return_encoded=True)
    feats = ss.encode(ss.process_input(x)[0])
    q2, i2, l2 = ss.rq(feats)
    b, n = feats.shape[:2]
    assert n == 12 and torch.equal(quantized, q2) and torch.equal(indices, i2.permute(1, 2, 0, 3).reshape(b, n, -1))     # 'g b n q -> b n (g q)'
    assert float(commit.sum()) == 0. and float(l2.sum()) == 0. and not quantized.requires_grad
    codes = ss(x, return_codes_only=True)
    assert torch.equal(codes, i2) and torch.equal(ss.tokenize(x), i2) and int(codes.min()) >= 0 and int(codes.max()) < 32
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


def test_soundstream_loss_breakdown_carries_the_lfq_losses(S):
    ss, x = _soundstream(S, with_discriminators=True, stft_discriminator=False, multi_spectral_recon_loss_weight=0)
    ss.train()
    ss.rq.dropout_index = lambda: 2
    seen = []
    hook = ss.rq.register_forward_hook(lambda mod, args, output: seen.append(output[2].detach()))
    total, (recon, multi_spectral, adversarial, feature, commitment) = ss(x, return_loss_breakdown=True)
    hook.remove()
    (losses,) = seen
    assert losses.shape == (1, 3) and bool((losses != 0).all())
    assert float(commitment.detach()) != 0. and torch.equal(commitment.detach(), losses.sum()) and bool(torch.isfinite(total))
    total.backward()
    assert float(ss.rq.rvqs[0].project_in.weight.grad.abs().max()) > 0 and bool(torch.isfinite(ss.encoder[0].conv.weight.grad).all())


def test_soundstream_denoising_path(S):
    """with_film=True next to the LFQ: the conditioned forward in eval mode and a training step with the loss breakdown"""
    ss, x = _soundstream(S, with_film=True, with_discriminators=True, stft_discriminator=False, multi_spectral_recon_loss_weight=0)
    target = x * 0.5
    with torch.no_grad():
        on = ss(x, target=target, is_denoising=True, return_recons_only=True)
        off = ss(x, target=target, is_denoising=False, return_recons_only=True)
        quantized, indices, commit = ss(x, target=target, is_denoising=True, return_encoded=True)
    assert on.shape == off.shape == (2, 1, 320 * 12) and not torch.equal(on, off) and float(commit.sum()) == 0.
    assert indices.shape == (2, 12, 3) and int(indices.min()) >= 0 and int(indices.max()) < 32
    ss.train()
    ss.rq.dropout_index = lambda: 2
    total, (recon, _, _, _, commitment) = ss(x, target=target, is_denoising=True, return_loss_breakdown=True)
    assert float(commitment.detach()) != 0. and float(recon.detach()) > 0 and bool(torch.isfinite(total))
    total.backward()
    for p in (ss.encoder_film.to_cond.weight, ss.rq.rvqs[0].project_in.weight, ss.encoder[0].conv.weight):
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
