"""CPU: the hyper-connection kernels' tests before any kernel runs.  The float64 restatement (tests/hc_restated.py) equals the oracle's hc_width /
hc_depth / layer_norm composed by hand to 1e-12, forward and autograd; the inputs of every row of the case matrix keep tanh, the stream norms and the
LayerNorm variance in the regime the tolerances assume; the restatement run in float32 stays within a tenth of every tolerance constant (that is how the
constants are set); the route queries name the documented variant for every row; the launchers refuse bad arguments on the host; the new symbols are
declared, bound and exported."""
import os
import re

import pytest
import torch

import audiolm_oracle as O
import hc_restated as H
from audiolm_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 10001
F64 = torch.float64
VARIANT = {'plain': -1, 'pf0': 0, 'pf1': 1, 'pf2': 2, 'gl': 3}


@pytest.fixture(autouse=True)
def four_threads():
    """the CPU reductions of the float32 run change their order with the thread count: the constants were measured with 4, so measure with 4"""
    n = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(n)


def _sd(hc):
    return {'norm.gamma': hc['gamma'], 'dynamic_alpha_fn': hc['Wa'], 'dynamic_alpha_scale': hc['sa'], 'static_alpha': hc['Aa'],
            'dynamic_beta_fn': hc['wb'], 'dynamic_beta_scale': hc['sb'], 'static_beta': hc['Bb']}


def _close(a, b, what):
    e = float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    assert e <= 1e-12, (what, e)


@pytest.mark.parametrize('S', [2, 3, 4])
def test_the_restatement_equals_the_oracle(S):
    B, N, D = 2, 7, 40
    inp = H.cast_inputs(H.make_inputs(S, D, B * N, seed=1), F64)
    R0, hc1, hc2, g2, y = inp['R0'], inp['hc1'], inp['hc2'], inp['g2'], inp['y']
    # forward: width (hc1) -> depth -> width (hc2) + LayerNorm, and the final stream sum + LayerNorm
    bs = lambda R_tok: H.to_streams(R_tok, B, N).reshape(B * S, N, D)
    tok = lambda t: t.reshape(B * N, *t.shape[2:])
    x_o, Rp_o, beta_o = O.hc_width(_sd(hc1), '', bs(R0), S)
    w0 = H.width(R0, hc1)
    _close(w0['x'], tok(x_o), 'x')
    _close(w0['Rp'], tok(Rp_o), 'Rp')
    _close(w0['beta'], tok(beta_o), 'beta')
    R1_o = O.hc_depth(y.view(B, N, D), Rp_o, beta_o)                      # (b s) n d
    R1 = H.depth(R0, w0['alpha'], w0['beta'], y)
    _close(H.to_streams(R1, B, N).reshape(B * S, N, D), R1_o, 'depth')
    fin = H.final(R0, w0['alpha'], w0['beta'], y, g2)
    xs_o = R1_o.reshape(B, S, N, D).sum(1)
    _close(fin['xs'], tok(xs_o), 'xs')
    _close(fin['xn'], tok(O.layer_norm(xs_o, g2)), 'final xn')
    # the record's fields are what their names say
    _close(w0['alpha'], torch.tanh(w0['a_pre']) * hc1['sa'] + hc1['Aa'], 'alpha of a_pre')
    _close(w0['beta'], torch.tanh(w0['b_pre']) * hc1['sb'] + hc1['Bb'], 'beta of b_pre')
    _close(w0['rn'], 1.0 / R0.norm(dim=-1), 'rn')
    # backward: autograd of the oracle's composite against backward(), every restriction of it
    G, dbeta, dxn, extra, dx, gb, xb = (inp[k] for k in ('G', 'dbeta', 'dxn', 'extra', 'dx', 'gb', 'xb'))
    beta_k = w0['beta']
    for case in ('ln_ex', 'ln', 'dx', 'g_bcast', 'r_bcast'):
        leaf = (xb if case == 'r_bcast' else inp['R1']).clone().requires_grad_(True)
        R_tok = leaf.unsqueeze(1).expand(-1, S, -1) if case == 'r_bcast' else leaf
        p = {k: v.clone().requires_grad_(True) for k, v in hc2.items()}
        lng = g2.clone().requires_grad_(True)
        x_o, Rp_o, beta_o = O.hc_width(_sd(p), '', bs(R_tok), S)
        Gs = gb.unsqueeze(1).expand(-1, S, -1) if case == 'g_bcast' else G
        L = (tok(Rp_o) * Gs).sum() + (tok(beta_o) * dbeta).sum()
        if case in ('ln_ex', 'ln'):
            L = L + (tok(O.layer_norm(x_o, lng)) * dxn).sum() + ((tok(x_o) * extra).sum() if case == 'ln_ex' else 0.)
        else:
            L = L + (tok(x_o) * dx).sum()
        L.backward()
        kw = dict(ln_gamma=g2, dxn=dxn, extra=extra if case == 'ln_ex' else None) if case in ('ln_ex', 'ln') else dict(dx=dx)
        r = H.backward(xb if case == 'r_bcast' else inp['R1'], hc2, gb if case == 'g_bcast' else G, dbeta, y_k=None if case == 'r_bcast' else y,
                       beta_k=beta_k, r_bcast=case == 'r_bcast', g_bcast=case == 'g_bcast', dsum_scale=H.DSUM_SCALE, **kw)
        if case == 'r_bcast':
            _close(r['dsum'], H.DSUM_SCALE * leaf.grad, case + ' dsum')
        else:
            _close(r['dR'], leaf.grad, case + ' dR')
            _close(r['dy'], torch.einsum('mt,mtd->md', beta_k, leaf.grad), case + ' dy')
            _close(r['dbeta_out'], (leaf.grad * y.unsqueeze(1)).sum(-1), case + ' dbeta')
        for k in H.HC_KEYS:
            _close(r['grads'][k], p[k].grad, f'{case} grad {k}')
        if case in ('ln_ex', 'ln'):
            _close(r['grads']['ln'], lng.grad, case + ' grad ln')
        # the absolute-sum scales bound the sums they belong to
        for k in H.ABS_SUM_KEYS:
            assert bool((r['scale'][k] >= r['grads'][k].abs() * (1 - 1e-12)).all()), (case, k)
    # mode 1: the depth connection's backward alone
    r = H.backward(None, None, G, None, y_k=y, beta_k=beta_k, width_part=False)
    yl, bl = y.clone().requires_grad_(True), beta_k.clone().requires_grad_(True)
    (H.depth(R0, w0['alpha'], bl, yl) * G).sum().backward()
    _close(r['dy'], yl.grad, 'mode 1 dy')
    _close(r['dbeta_out'], bl.grad, 'mode 1 dbeta')


def _launches(D):
    return [H.tokens(D)] + [b * n for b, n in H.small_launches(D)]


@pytest.mark.parametrize('S,D', H.ROWS)
def test_inputs_and_float32_deviation_of_every_row(S, D):
    """The inputs: pre-activation std in [0.2, 0.8] (tanh neither linear nor saturated), no stream norm below 1e-3 of the mean norm, LayerNorm variance
    above 1e-3 -- for the three stream tensors a width connection is run on.  The constants: the float32 CPU run of the restatement deviates from the
    float64 run by at most TOL / 10, in the measures the GPU tests use, at the token counts the GPU tests use."""
    for M in _launches(D):
        inp = H.make_inputs(S, D, M)
        for name, c in H.input_conditions(inp).items():
            if M > 100:                                                     # (a standard deviation over S (S + 2) values of one token says nothing)
                assert 0.2 <= c['pre_std'] <= 0.8, (M, name, c)
            assert c['min_norm'] >= 1e-3 and c['min_var'] >= 1e-3, (M, name, c)
        for t in (inp['R0'], inp['R1'], inp['y'], inp['G'], inp['dxn'], inp['extra']):
            assert torch.equal(t, t.to(torch.bfloat16).float())             # both storage types read the same values
        dev = H.deviations(H.all_outputs(inp, torch.float32), H.all_outputs(inp, F64))
        for k, v in dev.items():
            assert v <= H.tolerances(M)[k] / 10, (M, k, v, H.tolerances(M)[k])


def test_token_counts_turn_every_loop_three_times():
    for S, D in H.ROWS:
        M, tp = H.tokens(D), H.tpb(D)
        niter = -(-M // tp)
        assert niter >= 3 * H.MAX_RESIDENT + 1 and (tp == 1 or M % tp != 0)
        assert all(niter % (256 * occ) != 0 for occ in range(1, 9))
        (Ba, Na), (Bb, Nb) = H.factorisations(D)
        assert Ba * Na == M and Bb * Nb == M and Na > H.MAX_RESIDENT * tp and Nb == 37
        for occ in range(1, 9):                                             # the carry of the (b, n) walk: stride >= N, and N does not divide it
            stride = 256 * occ * tp
            assert stride // Nb >= 1 and stride % Nb != 0
        # without a device the occupancy query falls back to 2 workgroups on 256 CUs; with one the partial rows are capped at 4 x 256 workgroups
        for mode, lnf in ((2, 0), (2, 1), (3, 1)):
            for bf in (0, 1):
                rows = _lib.query('alm_hc_partial_rows', mode, lnf, bf, S, M, D)
                assert rows % tp == 0 and 256 * tp <= rows <= 1024 * tp and 3 * (rows // tp) <= niter, (S, D, mode, lnf, bf, rows)


def _pf_passes(niter, grid, block, brk):
    """the two-fold unrolled loop of the prefetching kernels (hc_fwd_kernel / hc_bwd_kernel, PF and GL) for one workgroup: the passes it PROCESSES, in
    order (a pass >= niter is only ever prefetched, at a clamped token).  brk(it) is the loop's middle exit test."""
    done, it = [], block
    while it < niter:
        done.append(it)
        if brk(it):
            break
        done.append(it + grid)
        it += 2 * grid
    return done


def test_the_prefetch_loop_schedule_processes_every_pass_once_and_none_beyond():
    """An emulation of the loop schedule, not of the kernel.  With the shipped exit `it + grid >= niter` the workgroups of any grid process passes
    0 .. niter - 1 once each.  With `>` in its place, whenever niter // grid is odd the workgroup niter % grid meets `it + grid == niter` and goes on to
    process pass niter -- with one token per pass that is token M, whose loads are clamped to token 0 (counted twice in the parameter gradients) and
    whose stores land one token behind every output; that mutant is therefore not run on a device.  The equality is met by the one-token and the
    (TPB + 1)-token launch of every row (niter = grid = 1 or 2); the full token counts have an even quotient for every grid up to 1536 workgroups."""
    shipped = lambda niter, grid: sorted(p for b in range(grid) for p in _pf_passes(niter, grid, b, lambda it: it + grid >= niter))
    mutant = lambda niter, grid: sorted(p for b in range(grid) for p in _pf_passes(niter, grid, b, lambda it: it + grid > niter))
    for niter in sorted({-(-H.tokens(D) // H.tpb(D)) for _, D in H.ROWS} | {1, 2, 3, 512, 513, 768, 1024, 1400}):
        for grid in sorted({min(niter, 256 * occ) for occ in range(1, 9)}):
            assert shipped(niter, grid) == list(range(niter)), (niter, grid)
            assert mutant(niter, grid) == list(range(niter + ((niter // grid) & 1))), (niter, grid)
    for _, D in H.ROWS:
        for B, N in H.small_launches(D):
            niter = -(-B * N // H.tpb(D))
            assert niter in (1, 2) and mutant(niter, niter) == list(range(niter + 1))


def _variant(kind, S, D, B, N, bf, aligned16=1):
    mode, lnf, bc, rbc, dR, dsum = {'depth': (1, 0, 0, 0, 0, 0), 'depth_bcast': (1, 0, 1, 0, 0, 0), 'width_dx': (2, 0, 0, 0, 1, 0),
                                    'width_ln': (2, 1, 0, 0, 1, 0), 'fused_ln': (3, 1, 0, 0, 1, 0), 'bcast': (2, 0, 1, 0, 1, 0),
                                    'rbcast_sum': (2, 0, 0, 1, 0, 1)}[kind]
    return _lib.query('alm_hc_bwd_variant', mode, lnf, int(bf), S, B, N, D, bc, rbc, dR, dsum, D, aligned16)


def test_route_queries_name_the_documented_variant_for_every_row():
    seen_f, seen_b = set(), set()
    for S, D in H.ROWS:
        for B, N in H.factorisations(D) + H.small_launches(D):
            for bf in (False, True):
                assert _lib.query('alm_hc_fwd_prefetch', int(bf), 0, D) == int(H.expected_fwd_prefetch(D, bf))
                assert _lib.query('alm_hc_fwd_prefetch', int(bf), 1, D) == 0
                seen_f.add((H.expected_fwd_prefetch(D, bf), H.wpt(D), S))
                for kind in ('depth', 'depth_bcast', 'width_dx', 'width_ln', 'fused_ln', 'bcast', 'rbcast_sum'):
                    want = H.expected_bwd_variant(kind, S, D, bf)
                    assert _variant(kind, S, D, B, N, bf) == VARIANT[want], (kind, S, D, B, N, bf)
                    seen_b.add((want, H.wpt(D), S))
                assert _variant('fused_ln', S, D, B, N, bf, aligned16=0) == VARIANT[H.expected_bwd_variant('fused_ln', S, D, bf, aligned16=False)]
    # together: forward PF and non-PF, backward plain / bc 0 / 1 / 2 for every (waves per token, S); GL where it exists
    for w in (1, 2, 4):
        for S in (2, 3, 4):
            assert {(True, w, S), (False, w, S)} <= seen_f
            assert {(v, w, S) for v in ('plain', 'pf0', 'pf1', 'pf2')} <= seen_b
    assert ('gl', 4, 4) in seen_b and not any(v == 'gl' and (w, S) != (4, 4) for v, w, S in seen_b)
    # requests the prefetching kernels cannot serve go to the plain kernel: both operands broadcast; stream-tensor R with dsum / without dR
    assert _lib.query('alm_hc_bwd_variant', 2, 0, 1, 4, 3, 2072, 1024, 1, 1, 0, 1, 1024, 1) == -1
    assert _lib.query('alm_hc_bwd_variant', 2, 0, 1, 4, 3, 2072, 1024, 0, 0, 1, 1, 1024, 1) == -1
    assert _lib.query('alm_hc_bwd_variant', 2, 0, 1, 4, 3, 2072, 1024, 0, 0, 0, 1, 1024, 1) == -1
    # ... and so does a tensor beyond the 32-bit byte offsets of the prefetching kernels (sizes only: nothing is launched)
    assert _lib.query('alm_hc_bwd_variant', 3, 1, 1, 4, 64, 8192, 1024, 0, 0, 1, 0, 1024, 1) == -1
    assert _lib.query('alm_hc_bwd_variant', 3, 1, 1, 4, 3, 2072, 1024, 0, 0, 1, 0, 1 << 20, 1) == -1


X = 0x7f0000001000                                                           # a non-NULL, 4096-byte aligned address that is never dereferenced on the host


def _fwd(**kw):
    a = dict(R_in=X, rin_bcast=0, r_bf16=0, y=X, ldy=64, coef_prev=X, R_out=X, hp=[X] * 7, ln=X, x=X, ldx=64, xn=X, ldxn=64, xn32=None, mean=X, rstd=X,
             coef=X, xs=X, mode=3, B=2, S=4, N=3, D=64)
    a.update(kw)
    return _lib.query('alm_hc_fwd', a['R_in'], a['rin_bcast'], a['r_bf16'], a['y'], a['ldy'], a['coef_prev'], a['R_out'], *a['hp'], a['ln'], a['x'], a['ldx'],
                      a['xn'], a['ldxn'], a['xn32'], a['mean'], a['rstd'], a['coef'], a['xs'], a['mode'], a['B'], a['S'], a['N'], a['D'], None)


def _bwd(**kw):
    a = dict(dRn=X, bcast=0, r_bf16=0, dx=None, lddx=0, dxn=X, lddxn=64, extra=X, ldex=64, mean=X, rstd=X, ln=X, R=X, r_bcast=0, coef=X, dbeta=X,
             hp=[X] * 5, dR=X, dsum=None, scale=1.0, partial=X, y=X, ldy=64, coef_prev=X, dy=X, lddy=64, dbo=X, mode=3, B=2, S=4, N=3, D=64)
    a.update(kw)
    return _lib.query('alm_hc_bwd', a['dRn'], a['bcast'], a['r_bf16'], a['dx'], a['lddx'], a['dxn'], a['lddxn'], a['extra'], a['ldex'], a['mean'], a['rstd'],
                      a['ln'], a['R'], a['r_bcast'], a['coef'], a['dbeta'], *a['hp'], a['dR'], a['dsum'], a['scale'], a['partial'], a['y'], a['ldy'],
                      a['coef_prev'], a['dy'], a['lddy'], a['dbo'], a['mode'], a['B'], a['S'], a['N'], a['D'], None)


def test_the_launchers_refuse_on_the_host():
    """ALM_ERR_BAD_ARG comes back on a machine without a device: the check sits in front of the launch (and of the occupancy query)"""
    for f in (_fwd, _bwd):
        for kw in (dict(B=0), dict(N=0), dict(B=-1), dict(N=-3), dict(D=0), dict(D=66), dict(D=1028), dict(mode=0), dict(mode=4), dict(mode=6), dict(mode=7),
                   dict(mode=-1), dict(ldy=66)):
            assert f(**kw) == BAD, (f.__name__, kw)
    assert _bwd(mode=5) == BAD
    # base pointers below the alignment of the vector accesses: 16 bytes for fp32 rows and ln_gamma, 8 bytes for bf16 rows
    for k in ('R_in', 'R_out', 'xs', 'ln'):
        assert _fwd(**{k: X + 8}) == BAD and _fwd(**{k: X + 4}) == BAD, k
    assert _fwd(xn=None, xn32=X + 8, mode=5) == BAD
    for k in ('y', 'x', 'xn'):
        assert _fwd(**{k: X + 4}) == BAD, k
    for k in ('R_in', 'R_out'):
        assert _fwd(r_bf16=1, **{k: X + 4}) == BAD, k
    assert _fwd(r_bf16=1, rin_bcast=1, R_in=X + 8) == BAD                   # (the broadcast input is fp32 next to bf16 streams)
    for k in ('dRn', 'R', 'dR', 'ln'):
        assert _bwd(**{k: X + 8}) == BAD, k
    assert _bwd(dsum=X + 8) == BAD and _bwd(dxn=None, extra=None, dx=X + 8, lddx=64) == BAD
    for k in ('dxn', 'extra', 'y', 'dy'):
        assert _bwd(**{k: X + 4}) == BAD, k
    for k in ('dRn', 'R', 'dR'):
        assert _bwd(r_bf16=1, **{k: X + 4}) == BAD, k
    assert _bwd(r_bf16=1, bcast=1, dRn=X + 8) == BAD and _bwd(r_bf16=1, r_bcast=1, R=X + 8) == BAD
    # the queries answer "plain" / "no prefetch" for what the launchers refuse
    assert _lib.query('alm_hc_bwd_variant', 3, 1, 1, 4, 0, 37, 1024, 0, 0, 1, 0, 1024, 1) == -1
    assert _lib.query('alm_hc_bwd_variant', 4, 1, 1, 4, 2, 37, 1024, 0, 0, 1, 0, 1024, 1) == -1
    assert _lib.query('alm_hc_fwd_prefetch', 1, 0, 1028) == 0 and _lib.query('alm_hc_fwd_prefetch', 1, 0, 0) == 0


def test_the_queries_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read()
    lib = _lib.load()
    for name in ('alm_hc_fwd_prefetch', 'alm_hc_bwd_variant'):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} is not declared in include/audiolm_hip.h'
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(',')), name
        assert hasattr(lib, name), name
    from audiolm_pytorch_amd import ops
    assert callable(ops.hc_fwd_prefetch) and callable(ops.hc_bwd_variant) and set(ops.HC_BWD_VARIANTS.values()) == set(VARIANT)
