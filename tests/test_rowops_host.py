"""CPU: the tests of the row kernels (csrc/norm_act.hip) and of the loss tail (csrc/embed_ce.hip) before any kernel runs.  The float64 restatement
(tests/rowops_restated.py) equals float64 autograd of the textbook formulas to 1e-12; the restatement run in float32 stays within a tenth of every
tolerance constant over the whole case matrix (that is how the constants are set); every mutant -- a kernel that is wrong in one of the ways such kernels
go wrong -- run through the float32 model misses a tolerance tenfold on the chosen inputs; the launchers refuse bad arguments on the host; the symbols are
declared, bound and exported."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import rowops_restated as R
from audiolm_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ['alm_ln_partial_blocks', 'alm_layernorm_fwd', 'alm_layernorm_bwd', 'alm_colsum', 'alm_colsum_chunks', 'alm_colsum_partial', 'alm_geglu_fwd',
           'alm_geglu_bwd', 'alm_geglu_partial_blocks', 'alm_geglu_ln_fwd', 'alm_geglu_ln_bwd', 'alm_cross_entropy_fwd', 'alm_cross_entropy_bwd',
           'alm_reduce_sum']


@pytest.fixture(autouse=True)
def four_threads():
    """the CPU reductions of the float32 run change their order with the thread count: the constants were measured with 4, so measure with 4"""
    n = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(n)


def _close(a, b, what):
    e = float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    assert e <= 1e-12, (what, e)


# ------------------------------------------------------------------------------------------------ restatement == autograd of the textbook formula
@pytest.mark.parametrize('rows,D', [(3, 4), (7, 260)])
def test_layer_norm_equals_autograd(rows, D):
    i = R.cast(R.ln_inputs(rows, D, 0), F64)
    x, g = i['x'][:, :D].clone(), i['gamma'].clone()
    if rows >= 3:
        x[2, D // 2] = 7.0                                  # (the 1e4 outlier costs the 1e-12 comparison three digits; it is for the kernels)
    f = R.layer_norm_fwd(x, g)
    xl, gl = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    y = F.layer_norm(xl, (D,), weight=gl, bias=None, eps=R.LN_EPS)
    _close(f['y'], y.detach(), 'y')
    _close(f['mean'], x.mean(-1), 'mean')
    _close(f['rstd'], (x.var(-1, unbiased=False) + R.LN_EPS).rsqrt(), 'rstd')
    (y * i['dy']).sum().backward()
    b = R.layer_norm_bwd(i['dy'], x, f['mean'], f['rstd'], g)
    _close(b['dx'], xl.grad, 'dx')
    _close(b['dgamma'], gl.grad, 'dgamma')
    _close(R.layer_norm_bwd(i['dy'], x, f['mean'], f['rstd'], g, i['extra'])['dx'], xl.grad + i['extra'], 'dx + extra')
    assert bool((b['dgamma_scale'] >= b['dgamma'].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('rows,I', [(4, 5), (7, 170)])
def test_geglu_ln_equals_autograd(rows, I):
    i = R.cast(R.geglu_inputs(rows, I), F64)
    ug = i['ug'].clamp(-12, 12)                             # (a gate of 1e4 costs the 1e-12 comparison digits; it is for the kernels)
    f = R.geglu_ln_fwd(i['ux'], ug, i['gamma'])
    xl, gl, gam = (t.clone().requires_grad_(True) for t in (i['ux'], ug, i['gamma']))
    h = F.gelu(gl) * xl
    hn = F.layer_norm(h, (I,), weight=gam, bias=None, eps=R.LN_EPS)
    _close(f['h'], h.detach(), 'h')
    _close(f['hn'], hn.detach(), 'hn')
    _close(f['mean'], h.detach().mean(-1), 'mean')
    _close(f['rstd'], (h.detach().var(-1, unbiased=False) + R.LN_EPS).rsqrt(), 'rstd')
    (hn * i['dhn']).sum().backward()
    b = R.geglu_ln_bwd(i['dhn'], i['ux'], ug, i['gamma'], f['mean'], f['rstd'])
    _close(b['dux'], xl.grad, 'du x half')
    _close(b['dug'], gl.grad, 'du gate half')
    _close(b['dgamma'], gam.grad, 'dgamma')
    # the standalone module
    x = torch.cat([i['ux'], ug], 1)
    xs = x.clone().requires_grad_(True)
    y = F.gelu(xs[:, I:]) * xs[:, :I]
    _close(R.geglu_fwd(x)[0], y.detach(), 'geglu y')
    (y * i['dhn']).sum().backward()
    _close(R.geglu_bwd(i['dhn'], x)[0], xs.grad, 'geglu dx')


def test_the_polynomial_is_abramowitz_stegun_7_1_26():
    """the fp32 model's cdf is the kernel's polynomial: within 1.5e-7 / 2 of the exact cdf in float64, and not the exact one"""
    v = torch.linspace(-12, 12, 48001, dtype=F64)
    (cp, pp), (ce, pe) = R.gauss_cdf_pdf(v, False), R.gauss_cdf_pdf(v, True)
    assert 1e-8 < float((cp - ce).abs().max()) <= 0.75e-7
    assert float((pp - pe).abs().max()) <= 1e-15


@pytest.mark.parametrize('ignore_index', [-1, 3])
def test_cross_entropy_equals_autograd(ignore_index):
    rows, C = 45, 21
    i = R.ce_inputs(rows, C, ignore_index)
    logits, labels = i['logits'].double(), i['labels']
    lab = torch.where(R.ce_ignored(labels, C, ignore_index), torch.full_like(labels, ignore_index), labels)   # F.cross_entropy refuses a label >= C
    f = R.cross_entropy_fwd(logits, labels, ignore_index)
    ll = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(ll, lab, reduction='none', ignore_index=ignore_index)
    _close(f['loss'], loss.detach(), 'loss')
    _close(f['lse'], torch.logsumexp(logits, -1), 'lse')
    w = torch.randn(rows, dtype=F64)                        # (row weights only to make the rows' gradients distinguishable; gscale is a scalar)
    (loss * w).sum().backward()
    d = R.cross_entropy_bwd(logits, labels, f['lse'], 1.0, ignore_index) * w.unsqueeze(1)
    assert bool(torch.isfinite(ll.grad).all())
    _close(d, ll.grad, 'dlogits')
    ign = R.ce_ignored(labels, C, ignore_index)
    assert int(ign.sum()) >= 3 and bool((f['loss'][ign] == 0).all()) and bool((d[ign] == 0).all())
    if ignore_index == 3:
        assert int((labels == 3).sum()) >= 1


def test_sums_equal_plain_sums():
    x = torch.randn(301, 7, dtype=F64)
    prev = torch.randn(7, dtype=F64)
    _close(R.colsum(x)[0], x.sum(0), 'colsum')
    _close(R.colsum(x, -2.5, prev)[0], prev - 2.5 * x.sum(0), 'colsum accumulate')
    _close(R.colsum(x, two_stage=False)[0], x.sum(0), 'colsum single stage')
    _close(R.colsum_partial(x, 5).sum(0), x.sum(0), 'partial')
    _close(R.reduce_sum(x.flatten(), 0.37)[0], 0.37 * x.sum(), 'reduce_sum')
    assert float(R.reduce_sum(x[:0].flatten())[0]) == 0.0
    assert [R.colsum_chunks(r) for r in (1, 128, 129, 1024, 1025, 3000)] == [_lib.query('alm_colsum_chunks', r) for r in (1, 128, 129, 1024, 1025, 3000)]


# ------------------------------------------------------------------------------------------------ the constants are ten times the float32 model's deviation
def test_every_tolerance_is_ten_times_the_float32_model():
    dev = R.all_deviations()
    assert set(dev) == set(R.TOL)
    for k, v in dev.items():
        print(f'{k:12s} model {v:.3g}  TOL {R.TOL[k]:.3g}')
        assert 0.0 < v <= R.TOL[k] / 10 * (1 + 1e-2), (k, v, R.TOL[k])
        assert R.TOL[k] <= 10.2 * v, (k, v, R.TOL[k])      # and no wider than that rule gives


def test_the_case_matrix_is_what_the_kernels_need():
    fw, bw = R.ln_fwd_cases(), R.ln_bwd_cases()
    for D in R.LN_DS:
        assert {c[0] for c in fw if c[1] == D} >= {1, 3, 37} and {c[0] for c in bw if c[1] == D} >= {1, 3, 37}
    for D in (260, 1028):
        assert {c[2:] for c in fw if c[1] == D and c[0] == 37} == set(R.LN_FWD_COMBOS)
    assert {c[2:5] for c in bw} == set(R.LN_BWD_COMBOS)
    assert {(c[4], c[6]) for c in bw} == {(0, 0), (0, 1), (1, 0), (1, 1)}                        # dgamma NULL and not, with both dx types
    assert all(_lib.query('alm_ln_partial_blocks', rows) * 4 < rows for rows in (2051, 4100)) and 4096 * 4 < 16389
    assert {c[1] % 4 for c in R.geglu_cases('fwd')} == {0, 1, 2, 3}
    assert all(rows > 2048 for rows in R.GEGLU_FWD_PIPE_ROWS) and all(rows > _lib.query('alm_geglu_partial_blocks', rows) for rows in R.GEGLU_BWD_PIPE_ROWS)
    assert 4099 * 513 > 8192 * 256 and 32773 > 8192 * 4


# ------------------------------------------------------------------------------------------------ mutants
def _caught(devs):
    """the largest deviation / tolerance over the cases and quantities"""
    return max(v / R.TOL[k] for d in devs for k, v in d.items())


@pytest.mark.parametrize('mutant', ['div_dm1', 'one_pass', 'eps_outside'])
def test_a_wrong_layer_norm_is_caught(mutant):
    small = [c for c in R.ln_fwd_cases() if c[0] <= 37]
    assert _caught(R.ln_fwd_dev(c, mutant=mutant) for c in small) >= 10, mutant


@pytest.mark.parametrize('mutant', ['drop4', 'div_ipad', 'pad_in_mean', 'tanh_gelu'])
def test_a_wrong_geglu_ln_forward_is_caught(mutant):
    small = [c for c in R.geglu_cases('fwd') if c[0] <= 19]
    assert _caught(R.geglu_fwd_dev(c, mutant=mutant) for c in small) >= 10, mutant
    if mutant == 'drop4':                                   # every width that is a multiple of 4 catches it on its own (19 rows: one gate there may be << 0)
        for c in small:
            if c[1] % 4 == 0 and c[0] == 19:
                assert _caught([R.geglu_fwd_dev(c, mutant=mutant)]) >= 10, c


def test_a_stale_prefetch_buffer_is_caught():
    small = [c for c in R.geglu_cases('bwd') if c[0] == 19]
    for c in small:
        if c[1] >= 4:
            assert _caught([R.geglu_bwd_dev(c, mutant='stale_stats')]) >= 10, c
    assert _caught([R.geglu_bwd_dev((1025, 5, 8, 0, 0), mutant='stale_stats')]) >= 10


@pytest.mark.parametrize('mutant', ['no_max', 'label_on_ignored'])
def test_a_wrong_cross_entropy_is_caught(mutant):
    small = [c for c in R.ce_cases() if c[0] <= 45]
    devs = [R.ce_dev(c, mutant=mutant) for c in small]
    assert _caught(devs) >= 10, mutant
    if mutant == 'no_max':
        assert _caught(devs) == math.inf                    # exp(300 + ..) overflows: without the max subtraction the row is inf / NaN


# ------------------------------------------------------------------------------------------------ launchers
def test_the_launchers_refuse_on_the_host():
    """every entry point checks its arguments before the launch: the refusal comes back on a machine without a GPU.  X is a non-null address that is never
    dereferenced (each call below has exactly one defect, rows > 0, and is refused for it)."""
    q, BAD, UNS, X = _lib.query, 10001, 10002, ctypes.c_void_p(4096)

    def each(name, good, defects, code=BAD):
        for i, v in defects:
            args = list(good)
            args[i] = v
            assert q(name, *args) == code, (name, i, v)

    # x, x_is_bf16, ldx, gamma, y, y_is_f32, ldy, xcopy, ldc, mean, rstd, rows, D, stream
    good = [X, 0, 264, X, X, 0, 268, X, 272, X, X, 5, 260, None]
    each('alm_layernorm_fwd', good, [(0, None), (3, None), (4, None), (9, None), (10, None), (2, 256), (6, 256), (8, 256), (2, 266), (6, 270), (8, 274),
                                     (12, 262), (12, 0)])
    each('alm_layernorm_fwd', [X, 0, 2060, X, X, 0, 2060, X, 2060, X, X, 5, 2048, None], [(12, 2052)], UNS)
    # dy, dy_is_f32, lddy, x, x_is_bf16, ldx, mean, rstd, gamma, extra, lde, dx, dx_is_bf16, lddx, dgamma_part, rows, D, stream
    good = [X, 0, 268, X, 0, 264, X, X, X, X, 264, X, 0, 272, X, 5, 260, None]
    each('alm_layernorm_bwd', good, [(0, None), (3, None), (6, None), (7, None), (8, None), (11, None), (2, 256), (5, 256), (10, 256), (13, 256), (2, 270),
                                     (16, 262), (16, 0)])
    f32 = list(good)
    f32[1] = 1                                                                  # an fp32 dy goes with an fp32 x and an fp32 dx only
    each('alm_layernorm_bwd', f32, [(4, 1), (12, 1)], UNS)
    each('alm_layernorm_bwd', [X, 0, 2060, X, 0, 2060, X, X, X, None, 0, X, 0, 2060, None, 5, 2048, None], [(16, 2052)], UNS)
    # u, ldu, gate_offset, gamma, out, ldo, mean, rstd, rows, inner, inner_pad, stream
    good = [X, 1400, 696, X, X, 696, X, X, 5, 681, 688, None]
    each('alm_geglu_ln_fwd', good, [(0, None), (3, None), (4, None), (6, None), (7, None), (1, 1376), (2, 680), (5, 684), (5, 698)])
    each('alm_geglu_ln_fwd', good, [(10, 692), (10, 680), (9, 0), (1, 1404), (2, 700)], UNS)
    each('alm_geglu_ln_fwd', [X, 6200, 3080, X, X, 3080, X, X, 5, 3075, 3072, None], [(10, 3080)], UNS)
    # dhn, lddh, u, ldu, gate_offset, gamma, mean, rstd, du, dgamma_part, rows, inner, inner_pad, stream
    good = [X, 704, X, 1400, 696, X, X, X, X, X, 5, 681, 688, None]
    each('alm_geglu_ln_bwd', good, [(0, None), (2, None), (5, None), (6, None), (7, None), (8, None), (1, 684), (1, 698), (3, 1376), (4, 680)])
    each('alm_geglu_ln_bwd', good, [(12, 692), (12, 680), (11, 0)], UNS)
    each('alm_geglu_ln_bwd', [X, 3080, X, 6200, 3080, X, X, X, X, None, 5, 3075, 3072, None], [(12, 3080)], UNS)
    # x, y, rows, inner, stream  /  dy, x, dx, rows, inner, stream
    each('alm_geglu_fwd', [X, X, 5, 7, None], [(0, None), (1, None)])
    each('alm_geglu_bwd', [X, X, X, 5, 7, None], [(0, None), (1, None), (2, None)])
    # in, in_is_bf16, ld, rows, cols, out, scale, accumulate, ws, stream
    each('alm_colsum', [X, 0, 70, 5, 65, X, 1.0, 0, None, None], [(0, None), (5, None), (2, 64)])
    # in, ld, rows, cols, ws, stream
    each('alm_colsum_partial', [X, 70, 200, 65, X, None], [(0, None), (4, None), (1, 64), (2, 0), (3, 0)])
    # logits, ld, labels, loss_rows, lse, rows, C, ignore_index, stream
    each('alm_cross_entropy_fwd', [X, 32, X, X, X, 5, 21, -1, None], [(0, None), (2, None), (3, None), (4, None), (1, 20), (6, 0)])
    # logits, ld, labels, lse, gscale, dlogits, ldd, rows, C, Cpad, ignore_index, stream
    each('alm_cross_entropy_bwd', [X, 32, X, X, X, X, 40, 5, 21, 24, -1, None],
         [(0, None), (2, None), (3, None), (4, None), (5, None), (1, 20), (8, 0), (9, 16), (6, 16)])
    # in, n, out, scale, stream
    each('alm_reduce_sum', [X, 5, X, 1.0, None], [(0, None), (2, None), (1, -1)])
    # rows <= 0 comes first: nothing to do is not an error
    assert q('alm_layernorm_fwd', None, 0, 0, None, None, 0, 0, None, 0, None, None, 0, 260, None) == 0
    assert q('alm_geglu_ln_fwd', None, 0, 0, None, None, 0, None, None, 0, 681, 688, None) == 0
    assert q('alm_cross_entropy_fwd', None, 0, None, None, None, 0, 21, -1, None) == 0


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} is not declared in include/audiolm_hip.h'
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(',')), name
        assert hasattr(lib, name), name
