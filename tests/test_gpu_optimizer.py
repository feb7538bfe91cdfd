"""Fused optimiser step (csrc/optim.hip, through the C ABI) vs torch.optim.Adam / AdamW + torch.nn.utils.clip_grad_norm_ on a real MI355X:
same parameters / gradients for several steps.  fp32 elementwise maths in a different association order: parameters agree to 2e-6
relative to their magnitude after 5 steps, the reported gradient norm to 1e-5."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(1024, 1024), (2730,), (3, 1025, 64), (17,), (1,), (128, 1024), (5, 7, 9)]
    return [torch.randn(*s, generator=g).cuda() for s in shapes]


@pytest.mark.parametrize('wd,max_norm', [(0., None), (0., 0.5), (1e-2, 0.5), (1e-2, None), (0., 1e9)])
def test_fused_adam_matches_torch(wd, max_norm):
    import audiolm_pytorch_amd as A
    ours = [torch.nn.Parameter(p.clone()) for p in _params(0)]
    ref = [torch.nn.Parameter(p.clone()) for p in _params(0)]
    o = A.get_optimizer(ours, lr=1e-3, wd=wd)
    if wd > 0:
        r = torch.optim.AdamW([{'params': [p for p in ref if p.ndim >= 2]}, {'params': [p for p in ref if p.ndim < 2], 'weight_decay': 0}],
                              lr=1e-3, weight_decay=wd, betas=(0.9, 0.99), eps=1e-8)
    else:
        r = torch.optim.Adam(ref, lr=1e-3, betas=(0.9, 0.99), eps=1e-8)
    for step in range(5):
        grads = _params(100 + step)
        for p, q, gr in zip(ours, ref, grads):
            p.grad = (gr * (3.0 if step % 2 else 0.01)).clone()
            q.grad = p.grad.clone()
        if max_norm is not None:
            n_ref = torch.nn.utils.clip_grad_norm_(ref, max_norm)
            n_ours = o.clip_grad_norm_(max_norm)
            assert abs(float(n_ours) - float(n_ref)) <= 1e-5 * float(n_ref)
        v0 = [p._version for p in ours]
        o.step()
        r.step()
        assert all(p._version > v for p, v in zip(ours, v0)), 'parameter version counters must advance (bf16 weight caches key on them)'
        for p, q in zip(ours, ref):
            err = float((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp(min=1e-30))
            assert err <= 2e-6, (step, tuple(p.shape), err)
    so, sr = o.state_dict()['state'], r.state_dict()['state']
    assert set(so[0].keys()) == set(sr[0].keys()) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert float(so[0]['step']) == float(sr[0]['step']) == 5.0


def test_fused_adam_skips_parameters_without_gradient():
    import audiolm_pytorch_amd as A
    ps = [torch.nn.Parameter(p.clone()) for p in _params(1)]
    o = A.get_optimizer(ps, lr=1e-2, wd=0.)
    ps[0].grad = torch.ones_like(ps[0])
    before = [p.detach().clone() for p in ps]
    o.step()
    assert not torch.equal(ps[0].detach(), before[0])
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps[1:], before[1:]))


def test_fused_adam_keeps_a_step_count_per_parameter():
    """torch.optim.Adam tracks `step` per parameter: a parameter whose gradient is None on some steps (a conditional head, a late-unfrozen
    weight) gets its own bias corrections.  Three steps where the second parameter only has a gradient on steps 2 and 3."""
    import audiolm_pytorch_amd as A
    base = _params(3)[:3]
    ours = [torch.nn.Parameter(p.clone()) for p in base]
    ref = [torch.nn.Parameter(p.clone()) for p in base]
    o = A.get_optimizer(ours, lr=3e-3, wd=0.)
    r = torch.optim.Adam(ref, lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        for i, (p, q) in enumerate(zip(ours, ref)):
            if i == 1 and step == 0:
                p.grad = q.grad = None
                continue
            gr = torch.randn(p.shape, generator=g).to(p.device)
            p.grad, q.grad = gr.clone(), gr.clone()
        o.step()
        r.step()
        for p, q in zip(ours, ref):
            err = float((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp(min=1e-30))
            assert err <= 2e-6, (step, tuple(p.shape), err)
    assert [float(o.state[p]['step']) for p in ours] == [float(r.state[q]['step']) for q in ref] == [3.0, 2.0, 3.0]


def _train_model(seed=0):
    import audiolm_pytorch_amd as A
    torch.manual_seed(seed)
    model = A.CoarseTransformer(dim=256, depth=2, num_semantic_tokens=100, codebook_size=64, num_coarse_quantizers=3, flash_attn=True).cuda()

    class Codec:
        rq_groups = 1
        num_quantizers = 8
    w = A.CoarseTransformerWrapper(transformer=model, codec=Codec(), unique_consecutive=False, mask_prob=0.)
    w.train()
    g = torch.Generator().manual_seed(7)
    data = dict(semantic_token_ids=torch.randint(0, 100, (2, 40), generator=g).cuda(), coarse_token_ids=torch.randint(0, 64, (2, 30, 3), generator=g).cuda())
    return model, w, data


@pytest.mark.parametrize('wd', [0., 1e-2])
def test_fused_adam_writes_the_packed_weight_images(monkeypatch, wd):
    """Round 4 (alm_opt_adam_pack_step): the optimiser step of a dense GEMM weight also writes its packed bf16 images, so the forward after a step
    does not re-pack.  Model A trains (forward, backward, fused step); model B -- same initial weights, never run forward, hence no packed images and
    the plain alm_opt_adam_step for every tensor -- receives A's gradients and takes the same steps: parameters bit-identical after every step (the two
    kernels share the arithmetic).  A packs its stack weights in the first forward only; the images the optimiser left in A's cache are bit-identical to
    a fresh pack of the updated masters; with ALM_FUSED_ADAM_PACK off every forward re-packs.  (Losses of two separate training runs are NOT compared:
    the embedding-gradient atomics make gradients differ in the last bit between runs, and Adam's first steps turn that into sign flips.)"""
    import audiolm_pytorch_amd as A
    from audiolm_pytorch_amd import core, ops
    real = ops.pack_weights_multi

    def counting(packs):
        # the stack's weights only (jobs with a row-major destination; the logit heads pack transposed images of their own and are not fused)
        return lambda jobs: (packs.append(sum(1 for j in jobs if j[1] is not None)), real(jobs))[1]

    monkeypatch.setattr(core, 'FUSED_ADAM_PACK', True)
    model_a, w_a, data = _train_model()
    model_b, _, _ = _train_model()
    model_b.load_state_dict(model_a.state_dict())                 # (the hyper-connection init draws from Python's `random`: two builds differ)
    opt_a = A.get_optimizer(model_a.parameters(), lr=1e-3, wd=wd)
    opt_b = A.get_optimizer(model_b.parameters(), lr=1e-3, wd=wd)
    packs, per_step = [], []
    monkeypatch.setattr(ops, 'pack_weights_multi', counting(packs))
    for step in range(3):
        n0 = sum(packs)
        loss = w_a(**data, return_loss=True)
        per_step.append(sum(packs) - n0)
        loss.backward()
        if step == 0:
            # one dense weight sits the first update out (a late-unfrozen layer): its step count then differs from its group's, the group's table entries
            # carry per-tensor counts -- the per-tensor bias-correction branch of alm_opt_adam_pack_step
            late = next(p for k, p in model_a.named_parameters() if 'to_q' in k and p.dim() == 2)
            late.grad = None
        for pa, pb in zip(model_a.parameters(), model_b.parameters()):
            pb.grad = None if pa.grad is None else pa.grad.detach().clone()
        na = opt_a.clip_grad_norm_(0.5)
        nb = opt_b.clip_grad_norm_(0.5)
        assert float(na) == float(nb)
        opt_a.step()
        opt_b.step()
        for (k, pa), pb in zip(model_a.named_parameters(), model_b.parameters()):
            assert torch.equal(pa, pb), (step, k)
        opt_a.zero_grad(set_to_none=True)
    assert per_step[0] > 0 and per_step[1:] == [0, 0], per_step            # packed once, kept current by the optimiser
    steps = {float(opt_a.state[p]['step']) for p in model_a.parameters() if p in opt_a.state}
    assert steps == {2.0, 3.0}, steps                                      # (the late weight: two updates)
    # the images the fused step left in the cache == a fresh pack of the final masters
    monkeypatch.setattr(ops, 'pack_weights_multi', real)
    checked = 0
    for key, entry in model_a.transformer._cache.store.items():
        if not (isinstance(key, tuple) and len(key) == 3 and key[2] in ('wq', 'wkv', 'wo', 'w1', 'w2')):
            continue
        stamp, (W, WT) = entry
        master = next(p for p in model_a.parameters() if p.data_ptr() == stamp[0])
        assert stamp == (master.data_ptr(), master._version, tuple(master.shape)), key
        if key[2] == 'w1':
            ref_W, ref_WT = core._pack_w1(master.detach(), *_inner(model_a))
        elif key[2] == 'w2':
            ref_W, ref_WT = core._pack_w2(master.detach(), *_inner(model_a))
        else:
            ref_W, ref_WT = core._pack_plain(master.detach())
        assert torch.equal(W, ref_W) and torch.equal(WT, ref_WT), key
        checked += 1
    assert checked >= 10, checked
    # the switch: off -> every forward after a step re-packs
    monkeypatch.setattr(core, 'FUSED_ADAM_PACK', False)
    model_c, w_c, _ = _train_model()
    opt_c = A.get_optimizer(model_c.parameters(), lr=1e-3, wd=wd)
    packs_c, per_step_c = [], []
    monkeypatch.setattr(ops, 'pack_weights_multi', counting(packs_c))
    for step in range(2):
        n0 = sum(packs_c)
        w_c(**data, return_loss=True).backward()
        per_step_c.append(sum(packs_c) - n0)
        opt_c.step()
        opt_c.zero_grad(set_to_none=True)
    assert all(n > 0 for n in per_step_c), per_step_c


def _inner(model):
    cfg = model.transformer.cfg
    return cfg.inner, cfg.inner_pad


# ---- through FusedAdam against the float64 restatement (tests/optim_restated.py): per element, with the bounds of tests/test_gpu_optim_kernels.py.  After
# every step the reference restarts from the GPU's own fp32 state, so one step's roundings are all there is to bound.

def _np(t):
    return t.detach().cpu().numpy().copy()


def _state_np(o, p):
    st = o.state[p]
    if len(st) == 0:
        z = _np(torch.zeros_like(p))
        return z, z.copy(), 0
    return _np(st['exp_avg']), _np(st['exp_avg_sq']), int(st['step'])


def _check_step(o, ps, before, grads, *, sumsq, max_norm, tag):
    """`before`: [(p, m, v, step)] read from the GPU before the step; every parameter with a gradient must now be within the per-element bounds"""
    import numpy as np
    import optim_restated as R
    worst = dict(p=0., m=0., v=0.)
    for i, (p, (p0, m0, v0, s0), g) in enumerate(zip(ps, before, grads)):
        group = next(gr for gr in o.param_groups if any(q is p for q in gr['params']))
        if g is None:
            assert np.array_equal(_np(p), p0), (tag, i)
            continue
        b1, b2 = group['betas']
        kw = dict(lr=group['lr'], beta1=b1, beta2=b2, eps=group['eps'], step=s0 + 1, wd=group['weight_decay'], decoupled=bool(group['decoupled_weight_decay']),
                  sumsq=sumsq, max_norm=max_norm or 0.)
        m1, v1, s1 = _state_np(o, p)
        assert s1 == s0 + 1, (tag, i)
        got = dict(p=_np(p).ravel(), m=m1.ravel(), v=v1.ravel())
        assert all(np.isfinite(a).all() for a in got.values()), (tag, i)
        # (the decoupled-decay factor as an fp32 hyper-parameter where 1 - lr wd is not exact in fp32: optim_restated.reference_and_ratios)
        _, r = R.reference_and_ratios(got, dict(p=p0, g=g, m=m0, v=v0), kw, 'fp32')
        for q in worst:
            worst[q] = max(worst[q], r[q])
    print(f'{tag:40s} GPU  m {worst["m"] * 4:5.2f}/4  v {worst["v"] * 6:5.2f}/6  p {worst["p"]:5.3f} of its bound')
    assert max(worst.values()) <= 1., (tag, worst)


def _run_steps(o, ps, grad_fn, steps, max_norm, tag):
    import numpy as np
    for it in range(steps):
        grads = grad_fn(it)
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g).cuda().reshape(p.shape)
        before = [(_np(p),) + _state_np(o, p) for p in ps]
        sumsq = None
        if max_norm is not None:
            norm = float(o.clip_grad_norm_(max_norm))
            want = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads if g is not None)))
            assert abs(norm - want) <= 1e-5 * want, (tag, it, norm, want)
            sumsq = norm * norm                                      # exact in float64, and its root is the fp32 norm the coefficient is made of
        o.step()
        _check_step(o, ps, before, grads, sumsq=sumsq, max_norm=max_norm, tag=f'{tag} step {it + 1}')


def test_fused_adam_130_parameters_in_one_group_against_the_restatement():
    """more than two batches of 64 tensors per launch, multi-chunk tensors at 0, 63, 64, 127, 128, empty parameters: clip_grad_norm_ + 3 steps"""
    import optim_restated as R
    from audiolm_pytorch_amd.optimizer import FusedAdam
    o, ps = _fused('x130')
    _run_steps(o, ps, lambda it: R.fused_grads('x130', it), 3, 0.5, 'FusedAdam x130')
    assert all(float(o.state[p]['step']) == 3.0 for p in ps)


def _fused(name):
    """the optimiser and parameters of optim_restated.FUSED[name] (tests/test_optim_host.py runs the fp32 model on the first step of each)"""
    import optim_restated as R
    from audiolm_pytorch_amd.optimizer import FusedAdam
    c = R.FUSED[name]
    ps = [torch.nn.Parameter(torch.from_numpy(p).cuda()) for p in R.fused_params(name)]
    return FusedAdam(ps, lr=c['lr'], betas=(0.9, 0.99), eps=1e-8, weight_decay=c['wd'], decoupled_weight_decay=c['decoupled']), ps


def test_fused_adam_l2_weight_decay_against_the_restatement():
    """FusedAdam(weight_decay=1e-2, decoupled_weight_decay=False): torch.optim.Adam's L2 decay (g += wd p), never run before"""
    import optim_restated as R
    o, ps = _fused('l2')
    sizes = R.FUSED['l2']['sizes']
    _run_steps(o, ps, lambda it: R.fused_grads('l2', it), 2, None, 'FusedAdam L2')
    _run_steps(o, ps, lambda it: [R.state(n, 6200 + 10 * it + i)['g'] for i, n in enumerate(sizes)], 1, 0.5, 'FusedAdam L2 clip')


def test_fused_adamw_at_the_hyper_parameters_training_uses():
    """lr 1e-3, wd 1e-2, decoupled: neither lr wd nor 1 - lr wd is exact in fp32.  Per element, clip_grad_norm_ + 2 steps"""
    import optim_restated as R
    o, ps = _fused('prod')
    _run_steps(o, ps, lambda it: R.fused_grads('prod', it), 2, 0.5, 'FusedAdamW lr 1e-3 wd 1e-2')


def test_fused_adam_with_a_group_of_empty_parameters_only():
    """a group whose every parameter has numel() == 0 has no chunk table: clip_grad_norm_() and step() pass it by (step() used to dereference the
    missing table), count its steps, and update the other group as if it were alone"""
    import optim_restated as R
    from audiolm_pytorch_amd.optimizer import FusedAdam
    empty = [torch.nn.Parameter(torch.zeros(0, device='cuda')), torch.nn.Parameter(torch.zeros(0, 4, device='cuda'))]
    full = [torch.nn.Parameter(torch.from_numpy(R.state(1025, 5600)['p']).cuda())]
    o = FusedAdam([{'params': empty}, {'params': full}], lr=R.HYPER['lr'], weight_decay=R.WD, decoupled_weight_decay=True)
    grads = [R.state(0, 1)['g'], R.state(0, 2)['g'], R.state(1025, 6600)['g']]
    _run_steps(o, empty + full, lambda it: grads, 1, 0.5, 'empty group')
    assert [float(o.state[p]['step']) for p in empty + full] == [1.0, 1.0, 1.0]
    alone = FusedAdam(empty, lr=R.HYPER['lr'])
    assert float(alone.clip_grad_norm_(0.5)) == 0.
    alone.step()
    assert all(float(alone.state[p]['step']) == 1.0 for p in empty)


@pytest.mark.parametrize('off', [1, 2, 3])
def test_fused_adam_on_offset_views_of_flat_buffers(off):
    """parameters and gradients that are views into flat buffers at 4, 8 and 12 bytes past a 16-byte boundary (the flat all-reduce buckets of data-parallel
    training hand out such gradients): the kernels' scalar paths, through the optimiser"""
    import numpy as np
    import optim_restated as R
    from audiolm_pytorch_amd.optimizer import FusedAdam
    sizes = (3, 4, 5, 1023, 1025, 16387)
    starts = np.cumsum([0] + [(n + 3) // 4 * 4 + 4 for n in sizes])
    flat_p = torch.zeros(int(starts[-1]) + 8, device='cuda')
    flat_g = torch.full((int(starts[-1]) + 8,), 777., device='cuda')
    ps = []
    for i, n in enumerate(sizes):
        view = flat_p[int(starts[i]) + off:int(starts[i]) + off + n]
        view.copy_(torch.from_numpy(R.state(n, 5200 + i)['p']))
        ps.append(torch.nn.Parameter(view))
        assert ps[-1].data_ptr() % 16 == 4 * off
    o = FusedAdam(ps, lr=R.HYPER['lr'], weight_decay=R.WD, decoupled_weight_decay=True)
    for it in range(2):
        grads = [R.state(n, 6300 + 10 * it + i)['g'] for i, n in enumerate(sizes)]
        for i, (p, g) in enumerate(zip(ps, grads)):
            gv = flat_g[int(starts[i]) + (off + 1) % 4:int(starts[i]) + (off + 1) % 4 + sizes[i]]
            gv.copy_(torch.from_numpy(g))
            p.grad = gv
        before = [(_np(p),) + _state_np(o, p) for p in ps]
        norm = float(o.clip_grad_norm_(0.5))
        want = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)))
        assert abs(norm - want) <= 1e-5 * want
        o.step()
        _check_step(o, ps, before, grads, sumsq=norm * norm, max_norm=0.5, tag=f'offset views +{off} step {it + 1}')
    live = torch.zeros_like(flat_p, dtype=torch.bool)
    for i, n in enumerate(sizes):
        live[int(starts[i]) + off:int(starts[i]) + off + n] = True
    assert not flat_p[~live].any()                                   # nothing written between the views


def test_fused_adam_all_zero_gradients_under_clipping():
    """norm 0 -> coef = min(1, 0.5 / 1e-6) = 1: nothing becomes non-finite, the moments stay 0 and the parameters move by the decoupled decay only"""
    import numpy as np
    import optim_restated as R
    from audiolm_pytorch_amd.optimizer import FusedAdam
    sizes = (7, 1025, 16385)
    ps = [torch.nn.Parameter(torch.from_numpy(R.state(n, 5300 + i)['p']).cuda()) for i, n in enumerate(sizes)]
    p0 = [_np(p) for p in ps]
    o = FusedAdam(ps, lr=R.HYPER['lr'], weight_decay=R.WD, decoupled_weight_decay=True)
    for p in ps:
        p.grad = torch.zeros_like(p)
    assert float(o.clip_grad_norm_(0.5)) == 0.
    o.step()
    for p, a in zip(ps, p0):
        got, want = _np(p), R.decayed_fp32(a, R.HYPER['lr'], R.WD, True)
        assert np.isfinite(got).all() and not _np(o.state[p]['exp_avg']).any() and not _np(o.state[p]['exp_avg_sq']).any()
        assert any(np.array_equal(got, w) for w in want)              # bit for bit fl(p c), c an fp32 decay factor
        assert not np.array_equal(got, a)


def test_fused_adam_applies_the_clip_of_the_last_norm():
    """clip_grad_norm_(), new gradients, clip_grad_norm_(), step(): the second norm's coefficient is the one applied"""
    import numpy as np
    import optim_restated as R
    from audiolm_pytorch_amd.optimizer import FusedAdam
    sizes = (5, 1025, 16385)
    ps = [torch.nn.Parameter(torch.from_numpy(R.state(n, 5400 + i)['p']).cuda()) for i, n in enumerate(sizes)]
    o = FusedAdam(ps, lr=R.HYPER['lr'])
    for i, p in enumerate(ps):
        p.grad = torch.from_numpy(R.state(sizes[i], 6400 + i)['g'] * np.float32(100.)).cuda()
    n1 = float(o.clip_grad_norm_(0.5))
    grads = [R.state(n, 6410 + i)['g'] for i, n in enumerate(sizes)]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).cuda()
    before = [(_np(p),) + _state_np(o, p) for p in ps]
    n2 = float(o.clip_grad_norm_(0.5))
    want = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)))
    assert abs(n2 - want) <= 1e-5 * want and n1 > 50 * n2
    o.step()
    _check_step(o, ps, before, grads, sumsq=n2 * n2, max_norm=0.5, tag='second clip')


@pytest.mark.parametrize('step_on_device', [False, True])
def test_checkpoints_interchange_with_torch_adam(step_on_device):
    """a torch.optim.Adam state_dict after 2 steps loaded into FusedAdam (once with `step` moved to the device, as map_location='cuda' leaves it): the
    third steps agree to the 2e-6 of test_fused_adam_matches_torch; then the reverse direction"""
    import copy

    import audiolm_pytorch_amd as A

    def grads(step):
        return [gr * (3.0 if step % 2 else 0.01) for gr in _params(200 + step)[1:]]

    def agree(xs, ys, tag):
        for p, q in zip(xs, ys):
            err = float((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp(min=1e-30))
            assert err <= 2e-6, (tag, tuple(p.shape), err)

    kw = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8)
    for first in ('torch', 'fused'):
        a = [torch.nn.Parameter(p.clone()) for p in _params(8)[1:]]
        make = {'torch': lambda ps: torch.optim.Adam(ps, **kw), 'fused': lambda ps: A.get_optimizer(ps, wd=0., **kw)}
        oa = make[first](a)
        for step in range(2):
            for p, gr in zip(a, grads(step)):
                p.grad = gr.clone()
            oa.step()
        b = [torch.nn.Parameter(p.detach().clone()) for p in a]
        ob = make['fused' if first == 'torch' else 'torch'](b)
        sd = copy.deepcopy(oa.state_dict())                    # (state_dict() hands out the live moment tensors, and load_state_dict keeps a tensor that needs no cast)
        if step_on_device and first == 'torch':
            for st in sd['state'].values():
                st['step'] = st['step'].cuda()
        ob.load_state_dict(sd)
        for p, q, gr in zip(a, b, grads(2)):
            p.grad, q.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
        agree(b, a, first)
        assert [float(ob.state[q]['step']) for q in b] == [3.0] * len(b)
        sa, sb = oa.state_dict()['state'], ob.state_dict()['state']
        for i in sa:
            agree([sb[i]['exp_avg'], sb[i]['exp_avg_sq']], [sa[i]['exp_avg'], sa[i]['exp_avg_sq']], first + ' moments')
