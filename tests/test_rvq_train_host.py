"""Host-side checks of the train-mode residual VQ: the restatement (tests/rvq_train_restated.py) against oracle/rvq_restated.py and against hand
arithmetic, the dropout-index recipe, the constructor options of the product module, the C ABI of csrc/rvq_train.hip, and the per-kernel references
of tests/test_gpu_rvq_train_kernels.py composed into one training step against TrainRVQ.forward + autograd.  No GPU."""
import os
import random
import re

import pytest
import torch

import rvq_restated
import rvq_train_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['alm_rvq_code_stats', 'alm_rvq_code_stats_ws_floats', 'alm_rvq_code_stats_chunk', 'alm_rvq_train_quantize', 'alm_rvq_train_quantize_blocks',
               'alm_rvq_ema_update', 'alm_rvq_expire', 'alm_rvq_kmeans_update', 'alm_rvq_train_bwd']


def _preset(rvq, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    for grp in rvq.state:
        for st in grp:
            st['embed'] = torch.randn(st['embed'].shape, generator=g).to(dtype)
            st['embed_avg'] = st['embed'].clone()
            st['initted'] = True


def test_eval_mode_equals_the_eval_restatement_bitwise():
    dim, groups, Q, C = 24, 2, 3, 17
    mine = R.TrainRVQ(dim=dim, groups=groups, num_quantizers=Q, codebook_size=C, dtype=torch.float32)
    _preset(mine, 1, torch.float32)
    ref = rvq_restated.GroupedResidualVQ(dim=dim, groups=groups, num_quantizers=Q, codebook_size=C).eval()
    for g, r in enumerate(ref.rvqs):
        for q, l in enumerate(r.layers):
            l._codebook.embed.copy_(mine.state[g][q]['embed'].unsqueeze(0))
            l._codebook.initted.fill_(True)
    x = torch.randn(2, 19, dim, generator=torch.Generator().manual_seed(2))
    out, idx, _ = mine.forward(x, training=False)
    rout, ridx, _ = ref(x)
    assert torch.equal(out, rout) and torch.equal(idx, ridx)


def test_dropout_index_follows_the_random_recipe():
    for Q, cutoff, mult in ((8, 1, 1), (8, 1, 2), (8, 0, 4), (4, 2, 1), (6, 1, 3)):
        for s in range(20):
            random.seed(s)
            got = R.dropout_index(Q, cutoff, mult)
            random.seed(s)
            k = random.Random(random.randint(0, int(1e7))).randrange(cutoff, Q)
            if mult != 1:
                k = -(-(k + 1) // mult) * mult - 1
            assert got == k and cutoff <= got < Q
            if mult != 1:
                assert (got + 1) % mult == 0
    assert R.dropout_index(1, 1, 1) == 0


def test_product_draws_the_same_dropout_index():
    from audiolm_pytorch_amd import soundstream as S
    for mult in (1, 2):
        rq = S.GroupedResidualVQ(dim=8, num_quantizers=8, codebook_size=4, quantize_dropout_multiple_of=mult)
        for s in range(10):
            random.seed(s)
            a = rq.dropout_index()
            random.seed(s)
            assert a == R.dropout_index(8, 1, mult)


def test_hand_computed_ema_step():
    """2 codes, 3 rows, d = 1, decay 0.5, no dropout, straight-through: rows 1, 2 -> code 0 (at 1), row 10 -> code 1 (at 9)"""
    rvq = R.TrainRVQ(dim=1, num_quantizers=1, codebook_size=2, decay=0.5, rotation_trick=False, threshold_ema_dead_code=0, eps=0.)
    st = rvq.state[0][0]
    st['initted'], st['embed'] = True, torch.tensor([[1.], [9.]], dtype=torch.float64)
    st['embed_avg'], st['cluster_size'] = torch.tensor([[2.], [9.]], dtype=torch.float64), torch.tensor([2., 1.], dtype=torch.float64)
    x = torch.tensor([[[1.], [2.], [10.]]], dtype=torch.float64)
    out, idx, losses = rvq.forward(x)
    assert idx.flatten().tolist() == [0, 0, 1]
    assert torch.equal(out.flatten(), torch.tensor([1., 1., 9.], dtype=torch.float64))
    assert abs(float(losses[0, 0]) - (0. + 1. + 1.) / 3) < 1e-15
    # n = (2, 1), s = (3, 10): cluster_size = (2, 1) / 2 + (2, 1) / 2 = (2, 1); embed_avg = (2, 9) / 2 + (3, 10) / 2 = (2.5, 9.5); eps = 0: smoothed = cluster_size
    assert torch.allclose(st['cluster_size'], torch.tensor([2., 1.], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(st['embed_avg'].flatten(), torch.tensor([2.5, 9.5], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(st['embed'].flatten(), torch.tensor([1.25, 9.5], dtype=torch.float64), atol=1e-15)


def test_expiry_resets_the_dead_codes():
    rvq = R.TrainRVQ(dim=1, num_quantizers=1, codebook_size=2, decay=0.5, rotation_trick=False, threshold_ema_dead_code=2, eps=0.,
                     sample_rows=lambda m, count: torch.tensor([2][:count]))
    st = rvq.state[0][0]
    st['initted'], st['embed'] = True, torch.tensor([[1.], [100.]], dtype=torch.float64)
    st['embed_avg'], st['cluster_size'] = torch.tensor([[2.], [100.]], dtype=torch.float64), torch.tensor([2., 1.], dtype=torch.float64)
    rvq.forward(torch.tensor([[[1.], [2.], [10.]]], dtype=torch.float64))
    # all three rows on code 0: cluster_size = (2.5, 0.5) -> code 1 is dead: embed = row 2 = 10, cluster_size = 2, embed_avg = 20
    assert st['cluster_size'].tolist() == [2.5, 2.] and st['embed'][1].item() == 10. and st['embed_avg'][1].item() == 20.


def test_straight_through_gradient_is_the_layer_count():
    dim, Q, C = 6, 4, 5
    for k in (0, 2, 3):
        rvq = R.TrainRVQ(dim=dim, num_quantizers=Q, codebook_size=C, rotation_trick=False)
        _preset(rvq, 3, torch.float64)
        x = torch.randn(2, 7, dim, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).requires_grad_()
        g_out = torch.randn(2, 7, dim, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        out, idx, losses = rvq.forward(x, k=k)
        out.backward(g_out)
        assert torch.allclose(x.grad, (k + 1) * g_out, rtol=0, atol=1e-12)
        assert bool((idx[..., k + 1:] == -1).all()) and bool((idx[..., :k + 1] >= 0).all()) and bool((losses[:, k + 1:] == 0).all())


def test_zero_row_has_no_nan_under_the_rotation_trick():
    rvq = R.TrainRVQ(dim=4, num_quantizers=2, codebook_size=3, rotation_trick=True)
    _preset(rvq, 6, torch.float64)
    x = torch.randn(1, 5, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    x[0, 2] = 0
    x.requires_grad_()
    out, _, losses = rvq.forward(x, k=1)
    (out.sum() + losses.sum()).backward()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())


def test_constructor_stores_the_options():
    from audiolm_pytorch_amd import soundstream as S
    rq = S.GroupedResidualVQ(dim=16, groups=2, num_quantizers=4, codebook_size=8, decay=0.9, commitment_weight=0.25, quantize_dropout_cutoff_index=2,
                             quantize_dropout_multiple_of=2, rotation_trick=False, threshold_ema_dead_code=3, kmeans_iters=5, eps=1e-4)
    assert (rq.decay, rq.commitment_weight, rq.quantize_dropout_cutoff_index, rq.quantize_dropout_multiple_of, rq.rotation_trick,
            rq.threshold_ema_dead_code, rq.kmeans_iters, rq.eps) == (0.9, 0.25, 2, 2, False, 3, 5, 1e-4)
    ss = S.SoundStream(channels=4, codebook_dim=16, codebook_size=8, rq_num_quantizers=4, use_local_attn=False, rq_ema_decay=0.8,
                       rq_commitment_weight=0.5, rq_quantize_dropout_multiple_of=2, rq_rotation_trick=False, quantize_dropout_cutoff_index=2)
    assert (ss.rq.decay, ss.rq.commitment_weight, ss.rq.quantize_dropout_multiple_of, ss.rq.rotation_trick, ss.rq.quantize_dropout_cutoff_index,
            ss.rq.threshold_ema_dead_code, ss.rq.kmeans_iters) == (0.8, 0.5, 2, False, 2, 2, 10)
    d = S.SoundStream(channels=4, codebook_dim=16, codebook_size=8, rq_num_quantizers=4, use_local_attn=False).rq
    assert (d.decay, d.commitment_weight, d.quantize_dropout_cutoff_index, d.quantize_dropout_multiple_of, d.rotation_trick, d.eps) == (0.95, 1., 1, 1, True, 1e-5)
    # the state_dict layout is the upstream one, unchanged
    assert sorted(k for k in ss.state_dict() if k.startswith('rq.rvqs.0.layers.0.')) == [
        'rq.rvqs.0.layers.0._codebook.' + n for n in ('cluster_size', 'embed', 'embed_avg', 'initted')]


def test_train_kernels_are_exported_and_declared():
    from audiolm_pytorch_amd import _lib
    lib = _lib.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\bint\s+(alm_\w+)\s*\(', src))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in declared and name in _lib.SIGNATURES, name
    assert _lib.query('alm_rvq_code_stats_chunk') > 0
    # hist [71][1024] + 2 x 1025 + perm 18000 + (18000 / chunk + 1024) x 512 words at the workload shape
    ch = _lib.query('alm_rvq_code_stats_chunk')
    assert _lib.query('alm_rvq_code_stats_ws_floats', 18000, 512, 1024) == 71 * 1024 + 2 * 1025 + 18000 + (18000 // ch + 1024) * 512
    assert _lib.query('alm_rvq_train_quantize_blocks', 0) == 0


@pytest.mark.parametrize('name', ['g2-rot-drop', 'expiry'])
def test_kernel_references_compose_into_the_training_step(name):
    """statistics -> quantize per layer -> EMA -> expiry -> backward, each by its per-kernel reference (R.code_stats_ref, quantize_ref, ema_update_ref,
    expire_ref, bwd_ref) on the indices TrainRVQ chose: the step of TrainRVQ.forward + autograd again, float64, max abs difference <= 1e-12.
    'g2-rot-drop' has two groups and a dropped layer (its index column is -1: a no-op in every reference); 'expiry' expires two codes per layer."""
    import test_gpu_rvq_train as T
    sc, seed, books, cs0, xs, gs = T.scenario_inputs(name)
    want = T.reference(name)['steps'][0]
    F64 = torch.float64
    M, Q, C, d = sc['b'] * sc['n'], sc['Q'], sc['C'], sc['dim'] // sc['groups']
    active = int((want['idx'][0, 0, 0] >= 0).sum())
    assert active == sc['k'] + 1
    cw, decay, eps, thr = 1., 0.95, 1e-5, 2.
    x, g_out, cs0 = xs[0].double().reshape(M, -1), gs[0].double().reshape(M, -1), cs0.double()
    expired = 0

    def same(what, a, b):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12, (name, what, float((a - b).abs().max()))

    for g in range(sc['groups']):
        xg, idx, E = x[:, g * d:(g + 1) * d], want['idx'][g].reshape(M, Q), torch.stack(books[g]).double()
        resid, out, losses, stats = xg, torch.zeros(M, d, dtype=F64), [], []
        for q in range(Q):
            stats.append(R.code_stats_ref(resid, idx[:, q], C))
            resid, out, loss, _ = R.quantize_ref(resid, idx[:, q], E[q], out, cw / (M * d), sc['rotation'])
            losses.append(loss)
        same('out', out, want['out'].reshape(M, -1)[:, g * d:(g + 1) * d])
        same('losses', torch.stack(losses), want['losses'][g])
        assert all(float(l) == 0 for l in losses[active:]) and all(float(n.sum()) == 0 for n, _ in stats[active:])
        for q in range(active):
            cs, ea, em, dead = R.ema_update_ref(cs0, E[q] * cs0[:, None], *stats[q], decay, eps, thr)
            if dead.numel():
                expired += dead.numel()
                cs, ea, em = R.expire_ref(dead, T.fixed_rows(M, dead.numel()), xg, idx, E, q, sc['rotation'], thr, cs, ea, em)
            st = want['state'][g][q]
            same(f'cluster_size {q}', cs, st['cluster_size']), same(f'embed_avg {q}', ea, st['embed_avg']), same(f'embed {q}', em, st['embed'])
        coef = torch.tensor([2 * cw / (M * d)] * Q, dtype=F64)       # d(sum of the losses) / d(loss_q) = 1
        same('dx', R.bwd_ref(xg, idx, E, g_out[:, g * d:(g + 1) * d], coef, sc['rotation']), want['dx'].reshape(M, -1)[:, g * d:(g + 1) * d])
    assert expired == (2 * active if sc['expiry'] else 0)
