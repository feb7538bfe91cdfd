"""Every kernel of csrc/rvq_train.hip on the MI355X, one `ops.rvq_*` call at a time, against the float64 per-kernel references of
tests/rvq_train_restated.py (checked without a GPU in tests/test_rvq_train_host.py).  Indices are inputs (random codes, no argmin, no ties).

Measure and bound: the rel-max measure and TOL = 2e-5 of tests/test_gpu_rvq_train.py (the same arithmetic with longer rows); `torch.equal` wherever the
source claims bit-identity.  No case needed a bound of its own.  Measured worst rel-max per kernel: DESIGN.md section 15.

Which case covers which path (K = columns per lane of the row kernels, row_k(d): 1, 2, 4, 8, 16 for d <= 64, 128, 256, 512, 1024):

  path                                                              | case
  ------------------------------------------------------------------+---------------------------------------------------------------------------
  row kernels K = 1 / 2 / 4 / 8 / 16, both edges and a ragged width | D_ALL = 64 | 65 100 128 | 129 200 256 | 257 384 512 | 513 1000 1024
    (the `lane + 64 k < d` tail guard: every d that is no             (quantize, backward); D_ONE = 64 | 100 | 200 | 384 | 1000 (expiry, and the
    multiple of 64)                                                   expiry against the chained quantize, bit for bit)
  quantize: part-filled last workgroup, a wave stopping mid-loop    | M = 77 (rows 64..76: wave 0 full, wave 1 stops after 5 rows, waves 2, 3 idle)
  quantize: skipped rows, strided `out`, zero |r|, zero |q|, u = -qh | about 10 % idx = -1; `out` = the second half of [M, 2 d]; three planted rows
  rvq_loss_finish_kernel, more than 256 partials                    | test_quantize_more_than_256_loss_partials (d = 65, M = 8225: 258 partials)
  backward: a workgroup of one row, strided x / g_out / dx          | M = 77 = 19 x 4 + 1; column slices of [M, 2 d]
  backward: g_out / coef absent, a dropped layer, a skipped layer    | the full cross given | None; idx[:, 2] = -1; idx[rows, 1] = -1
  expiry: q = 0 (no chain) and q = 2, invalid list entries           | q in {0, 2}; rows -1 and M in the list; a code -3 and a code C in the list
  rvq_ema_size_kernel with 1 / 1 / 2 / 3 / 4 passes of 256 codes     | (C, d) = (32, 16) (256, 64) (257, 300) (700, 256) (1024, 512)
    dead list across passes and waves, > 64 dead in one 256-block    | dead codes 0 63 64 255 256 511 512 C - 1 and 100..179; all dead (C = 700); none
  rvq_ema_embed_kernel, blockIdx.y > 0 with a partial last block     | (257, 300): 300 = 256 + 44; (1024, 512) is two full blocks
  rvq_kmeans_kernel, blockIdx.y > 0 with a partial last block        | (40, 300): 256 + 44; (40, 600): 2 x 256 + 88; with and without the embed outputs
  statistics: partial second column block                            | d = 300
  statistics: one code owns every row (33 chunks over 9 tiles)      | M = 2100, C = 1024, code 1023
  statistics: the LDS histogram at its limit / past it / no rows     | C = 8192 / C = 8193 raises / M = 0
"""
import functools

import pytest
import torch

import rvq_train_restated as R
from test_gpu_rvq_train import F32, F64, TOL, dev, gen, relmax

pytestmark = pytest.mark.gpu

D_ALL = [64, 65, 100, 128, 129, 200, 256, 257, 384, 512, 513, 1000, 1024]
D_ONE = [64, 100, 200, 384, 1000]
M_ROWS, C_CODES = 77, 37
SENTINEL = -7.25


def check(kernel, name, got, ref):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    e = relmax(got, ref)
    print(f'rvq-kernels | {kernel} | {name}: rel-max {e:.3e}')
    assert e <= TOL, (kernel, name, e)


@pytest.fixture(scope='module')
def ops():
    from audiolm_pytorch_amd import ops as _ops
    return _ops


def eighths(shape, g):
    """exactly representable in every precision: integers / 8 in [-1, 1], the first one 1"""
    v = torch.randint(-8, 9, shape, generator=g).float() / 8
    v[..., 0] = 1.
    return v


# ------------------------------------------------------------------------------------------------------------------------ 1. rvq_train_quantize

ZERO_R, ZERO_Q, ANTI = 3, 40, 76            # planted rows: zero residual | the selected code (5) is all zeros | r = -2 q (code 7), the LAST row


@functools.lru_cache(maxsize=None)
def quantize_case(d, rotation, M=M_ROWS, C=C_CODES):
    g = gen(1000 * d + rotation + M)
    E, resid = torch.randn(C, d, generator=g), torch.randn(M, d, generator=g)
    idx = torch.randint(0, C, (M,), generator=g)
    idx[[r for r in torch.randperm(M, generator=g).tolist() if r not in (ZERO_R, ZERO_Q, ANTI)][:M // 10]] = -1
    E[5], E[7] = 0., eighths((d,), g)
    idx[ZERO_R], idx[ZERO_Q], idx[ANTI] = 1, 5, 7
    resid[ZERO_R], resid[ANTI] = 0., -2 * E[7]
    wide = torch.randn(M, 2 * d, generator=g) + 3.
    wide[:, :d] = SENTINEL
    scale = 0.25 / (M * d)
    ref = R.quantize_ref(resid.double(), idx, E.double(), wide[:, d:].double(), scale, rotation)
    return E, resid, idx, wide, scale, tuple(t.detach() for t in ref)


def run_quantize(ops, d, rotation, M=M_ROWS):
    E, resid0, idx, wide0, scale, (resid_ref, out_ref, loss_ref, y_ref) = quantize_case(d, rotation, M)
    resid, wide, loss = resid0.to(dev()), wide0.to(dev()), torch.full((1,), 9., device=dev())
    ops.rvq_train_quantize(resid, idx.to(dev()), E.to(dev()), wide[:, d:], loss, scale, rotation)
    resid, wide, loss = resid.cpu(), wide.cpu(), loss.cpu()
    tag = f'd={d} rot={rotation} M={M}'
    assert bool(torch.isfinite(resid).all()) and bool(torch.isfinite(wide).all()) and bool(torch.isfinite(loss).all())
    check('quantize', f'{tag} resid', resid, resid_ref), check('quantize', f'{tag} out', wide[:, d:], out_ref)
    check('quantize', f'{tag} loss', loss, loss_ref.reshape(1))
    skip = idx < 0
    assert int(skip.sum()) == M // 10
    assert torch.equal(resid[skip], resid0[skip]) and torch.equal(wide[:, d:][skip], wide0[:, d:][skip])      # rows that take no part: bitwise untouched
    assert torch.equal(wide[:, :d], wide0[:, :d])                                                          # the other group's columns
    return E, resid0, resid, y_ref


@pytest.mark.parametrize('rotation', [0, 1])
@pytest.mark.parametrize('d', D_ALL)
def test_quantize(ops, d, rotation):
    E, resid0, resid, y_ref = run_quantize(ops, d, rotation)
    if rotation:
        # the reference itself: y = 0 for a zero residual and for a zero code (lam = 0); u + qh is EXACTLY 0 on the antiparallel row, where y = q
        assert float(y_ref[ZERO_R].abs().max()) == 0 and float(y_ref[ZERO_Q].abs().max()) == 0
        assert float((y_ref[ANTI] - E[7].double()).abs().max()) <= 1e-14
        assert torch.equal(resid[ZERO_R], resid0[ZERO_R]) and torch.equal(resid[ZERO_Q], resid0[ZERO_Q])
        check('quantize', f'd={d} antiparallel row', resid[ANTI], -3 * E[7].double())


def test_quantize_more_than_256_loss_partials(ops):
    assert ops._lib.query('alm_rvq_train_quantize_blocks', 8225) == 258
    run_quantize(ops, 65, 1, M=8225)


# ------------------------------------------------------------------------------------------------------------------------ 2. rvq_train_bwd

Q_LAYERS = 3


@functools.lru_cache(maxsize=None)
def chain_case(d, M=M_ROWS, C=C_CODES):
    """x (the first half of [M, 2 d]), idx [M, Q] (the last layer dropped, rows 10 / 33 / 76 without a code in layer 1), E [Q, C, d], g_out (the second
    half of [M, 2 d]), coef [Q]; row 5 of x is zero"""
    g = gen(7000 + d)
    E = torch.stack([torch.randn(C, d, generator=g) * 0.6 ** q for q in range(Q_LAYERS)])
    xw, gw = torch.randn(M, 2 * d, generator=g), torch.randn(M, 2 * d, generator=g)
    xw[5, :d] = 0.
    idx = torch.randint(0, C, (M, Q_LAYERS), generator=g)
    idx[:, 2] = -1
    idx[[10, 33, 76], 1] = -1
    coef = torch.rand(Q_LAYERS, generator=g) + 0.5
    return E, xw, gw, idx, coef


@functools.lru_cache(maxsize=None)
def bwd_reference(d, rotation, with_g, with_coef):
    E, xw, gw, idx, coef = chain_case(d)
    return R.bwd_ref(xw[:, :d].double(), idx, E.double(), gw[:, d:].double() if with_g else None, coef.double() if with_coef else None, rotation)


@pytest.mark.parametrize('with_coef', [True, False])
@pytest.mark.parametrize('with_g', [True, False])
@pytest.mark.parametrize('rotation', [0, 1])
@pytest.mark.parametrize('d', D_ALL)
def test_bwd(ops, d, rotation, with_g, with_coef):
    E, xw, gw, idx, coef = chain_case(d)
    xw, gw = xw.to(dev()), gw.to(dev())
    dxw = torch.full((M_ROWS, 2 * d), SENTINEL, device=dev())
    ops.rvq_train_bwd(xw[:, :d], idx.to(dev()), E.to(dev()), gw[:, d:] if with_g else None, coef.to(dev()) if with_coef else None, dxw[:, d:], rotation)
    dxw = dxw.cpu()
    assert bool(torch.isfinite(dxw).all())
    check('bwd', f'd={d} rot={rotation} g={with_g} coef={with_coef} dx', dxw[:, d:], bwd_reference(d, rotation, with_g, with_coef))
    assert bool((dxw[:, :d] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------ 3. rvq_expire

THR = 2.


def expire_buffers(d, g, C=C_CODES):
    return torch.rand(C, generator=g) * 9 + 3, torch.randn(C, d, generator=g), torch.randn(C, d, generator=g)


def run_expire(ops, d, rotation, q, codes, rows):
    E, xw, _, idx, _ = chain_case(d)
    cs0, ea0, em0 = expire_buffers(d, gen(9000 + d))
    cs, ea, em = cs0.to(dev()), ea0.to(dev()), em0.to(dev())
    ops.rvq_expire(torch.tensor(codes, dtype=torch.int32, device=dev()), len(codes), torch.tensor(rows, dtype=torch.int64, device=dev()), xw.to(dev())[:, :d],
                   idx.to(dev()), E.to(dev()), q, rotation, THR, cs, ea, em)
    ref = R.expire_ref(torch.tensor(codes), torch.tensor(rows), xw[:, :d].double(), idx, E.double(), q, rotation, THR, cs0.double(), ea0.double(), em0.double())
    return (cs0, ea0, em0), (cs.cpu(), ea.cpu(), em.cpu()), ref


@pytest.mark.parametrize('q', [0, 2])
@pytest.mark.parametrize('rotation', [0, 1])
@pytest.mark.parametrize('d', D_ONE)
def test_expire(ops, d, rotation, q):
    M, C = M_ROWS, C_CODES
    for codes, rows, valid in (([4, 9, 20, 30, 33], [10, -1, 76, M, 0], [4, 20, 33]),        # row 10 has no code in layer 1; rows -1 and M are skipped
                               ([4, C, -3], [1, 2, 5], [4])):                                # codes C and -3 are skipped; row 5 is the zero row
        (cs0, ea0, em0), (cs, ea, em), (cs_ref, ea_ref, em_ref) = run_expire(ops, d, rotation, q, codes, rows)
        check('expire', f'd={d} rot={rotation} q={q} embed', em[valid], em_ref[valid])
        assert torch.equal(ea[valid], em[valid] * THR) and cs[valid].tolist() == [THR] * len(valid)
        other = torch.ones(C, dtype=torch.bool)
        other[valid] = False
        assert torch.equal(cs[other], cs0[other]) and torch.equal(ea[other], ea0[other]) and torch.equal(em[other], em0[other])
        assert bool(torch.isfinite(em).all())


@pytest.mark.parametrize('rotation', [0, 1])
@pytest.mark.parametrize('d', D_ONE)
def test_expire_writes_the_bits_of_the_chained_quantize(ops, d, rotation):
    """rvq_row_y gives the same bits in every kernel that inlines it: the residual after q = 2 calls of rvq_train_quantize, and what rvq_expire
    recomputes for layer 2 from x, the indices and the codebooks, for 37 rows (rows 10, 33 and 76 skip layer 1; row 5 is zero)"""
    M, C, q = M_ROWS, C_CODES, 2
    E, xw, _, idx, _ = chain_case(d)
    Ed, idxd, x = E.to(dev()), idx.to(dev()), xw.to(dev())[:, :d]
    resid, out, loss = x.contiguous().clone(), torch.zeros(M, d, device=dev()), torch.zeros(1, device=dev())
    for l in range(q):
        ops.rvq_train_quantize(resid, idxd[:, l], Ed[l], out, loss, 1., rotation)
    rows = (torch.arange(C) * 2 + 2) % M                                                  # 2, 4, ..., 74, among them 10
    rows[:3] = torch.tensor([33, 76, 5])
    cs, ea, em = (t.to(dev()) for t in expire_buffers(d, gen(9100 + d)))
    ops.rvq_expire(torch.arange(C, dtype=torch.int32, device=dev()), C, rows.to(dev()), x, idxd, Ed, q, rotation, THR, cs, ea, em)
    assert not torch.equal(resid, x) and torch.equal(em, resid[rows.to(dev())])
    check('expire', f'd={d} rot={rotation} chained', em.cpu(), R.layer_residual_ref(xw[:, :d].double(), idx, E.double(), q, rotation)[rows])


# ------------------------------------------------------------------------------------------------------------------------ 4. rvq_ema_update

DECAY, EPS = 0.95, 1e-5
EMA_SHAPES = [(32, 16), (256, 64), (257, 300), (700, 256), (1024, 512)]


def ema_case(C, d, plan):
    """cluster_size is 6 (stays above 5.7), 1 (ends in [0.95, 1.45]) or 0 with n = 0 and a zero embed_avg (ends at 0): far from the threshold of 2"""
    g = gen(100 * C + d)
    n = torch.randint(0, 11, (C,), generator=g).float()
    s = torch.randn(C, d, generator=g) * n[:, None]
    low = torch.zeros(C, dtype=torch.bool)
    if plan == 'planted':
        low[[c for c in (0, 63, 64, 255, 256, 511, 512, C - 1) if c < C]] = True
        low[100:180] = True                                                               # 80 dead codes inside the first 256-block (none at C = 32)
        low |= torch.rand(C, generator=g) < 0.1
    elif plan == 'all':
        low[:] = True
    cs = torch.where(low, 1., 6.)
    zero = low & (torch.arange(C) % 3 == 0)
    cs[zero], n[zero], s[zero] = 0., 0., 0.
    ea = torch.randn(C, d, generator=g) * cs[:, None]
    return cs, ea, n, s, low


@pytest.mark.parametrize('C,d,plan,thr', [(C, d, 'planted', 2.) for C, d in EMA_SHAPES] + [(700, 256, 'all', 2.), (257, 300, 'none', 2.), (257, 300, 'planted', 0.)])
def test_ema_update(ops, C, d, plan, thr):
    cs0, ea0, n, s, low = ema_case(C, d, plan)
    cs_ref, ea_ref, em_ref, dead_ref = R.ema_update_ref(cs0.double(), ea0.double(), n.double(), s.double(), DECAY, EPS, thr)
    assert thr == 0 or float((cs_ref - thr).abs().min()) > 1e-3                           # the dead set is unambiguous (no threshold: nothing is dead)
    want = low.nonzero()[:, 0].tolist() if thr > 0 else []
    assert dead_ref.tolist() == want and bool((cs_ref == 0).any()) == bool(low.any())
    if plan == 'planted' and thr > 0:
        assert all(c in want for c in (0, 63, 64, 255, 256, 511, 512, C - 1) if c < C) and (C < 256 or sum(c < 256 for c in want) > 64)
    cs, ea, em = cs0.to(dev()), ea0.to(dev()), torch.full((C, d), SENTINEL, device=dev())
    dead = torch.full((1 + C + 8,), -77, dtype=torch.int32, device=dev())
    ops.rvq_ema_update(cs, ea, em, n.to(dev()), s.to(dev()), DECAY, EPS, thr, dead)
    dead = dead.cpu().tolist()
    assert dead[0] == len(want) and dead[1:1 + len(want)] == want and dead[1 + len(want):] == [-77] * (C + 8 - len(want))
    tag = f'C={C} d={d} {plan} thr={thr}'
    check('ema', f'{tag} cluster_size', cs, cs_ref), check('ema', f'{tag} embed_avg', ea, ea_ref), check('ema', f'{tag} embed', em, em_ref)
    assert bool(torch.isfinite(em).all())


# ------------------------------------------------------------------------------------------------------------------------ 5. rvq_kmeans_update

@pytest.mark.parametrize('with_outputs', [True, False])
@pytest.mark.parametrize('C,d', [(16, 4), (300, 256), (40, 300), (40, 600)])
def test_kmeans_update(ops, C, d, with_outputs):
    g = gen(50 * C + d)
    n = torch.randint(0, 9, (C,), generator=g).float()
    n[[1, C - 1]] = 0.
    empty = n == 0
    s, means0 = torch.randn(C, d, generator=g) * n[:, None], torch.randn(C, d, generator=g)
    means = means0.to(dev())
    outs = [torch.full((C, d), SENTINEL, device=dev()), torch.full((C, d), SENTINEL, device=dev()), torch.full((C,), SENTINEL, device=dev())]
    ops.rvq_kmeans_update(means, n.to(dev()), s.to(dev()), *(outs if with_outputs else ()))
    assert torch.equal(means.cpu()[empty], means0[empty]) and int(empty.sum()) >= 2
    check('kmeans', f'C={C} d={d} means', means, R.kmeans_update_ref(means0.double(), n.double(), s.double()))
    if with_outputs:
        assert torch.equal(outs[0], means) and torch.equal(outs[1], means * n.to(dev())[:, None]) and torch.equal(outs[2].cpu(), n)
    else:
        assert all(bool((t == SENTINEL).all()) for t in outs)


# ------------------------------------------------------------------------------------------------------------------------ 6. rvq_code_stats

def stats_against_index_add(ops, wide, idx, C):
    """the asserts of test_gpu_rvq_train.test_code_stats_against_index_add: counts exact, sums within TOL, empty codes exactly zero, two runs the same bits"""
    d = wide.shape[1] // 2
    n_ref, s_ref = R.code_stats_ref(wide[:, d:].double(), idx, C)
    wd, idd = wide.to(dev()), idx.to(dev())
    runs = [ops.rvq_code_stats(wd[:, d:], idd, C) for _ in range(2)]
    n, s = runs[0]
    assert torch.equal(n.cpu().double(), n_ref)
    assert bool((s[n == 0] == 0).all())
    check('stats', f'M={wide.shape[0]} d={d} C={C} s', s, s_ref)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    return n.cpu()


def test_code_stats_partial_second_column_block(ops):
    g = gen(300)
    M, d, C = 197, 300, 40
    idx = torch.randint(0, C - 5, (M,), generator=g)
    idx[torch.randperm(M, generator=g)[:M // 10]] = -1
    n = stats_against_index_add(ops, torch.randn(M, 2 * d, generator=g), idx, C)
    assert int((n == 0).sum()) >= 5


def test_code_stats_fully_collapsed_codebook(ops):
    g = gen(2100)
    M, d, C = 2100, 16, 1024
    idx = torch.full((M,), C - 1)
    idx[torch.randperm(M, generator=g)[:20]] = -1
    rows = M - 20
    assert -(-rows // ops.rvq_code_stats_chunk()) == 33 and -(-M // 256) == 9
    n = stats_against_index_add(ops, torch.randn(M, 2 * d, generator=g), idx, C)
    assert n[C - 1] == rows and int((n == 0).sum()) == C - 1


def test_code_stats_at_the_histogram_limit(ops):
    g = gen(8192)
    M, d, C = 300, 16, 8192
    idx = torch.randint(0, C, (M,), generator=g)
    idx[:4] = torch.tensor([0, C - 1, C - 1, -1])
    wide = torch.randn(M, 2 * d, generator=g)
    n = stats_against_index_add(ops, wide, idx, C)
    assert n[C - 1] >= 2 and int((n == 0).sum()) >= C - M
    with pytest.raises(ops._lib.AlmError, match='ALM_ERR_UNSUPPORTED'):
        ops.rvq_code_stats(wide.to(dev())[:, d:], idx.to(dev()), C + 1)


def test_code_stats_without_rows(ops):
    d, C = 16, 40
    wide = torch.zeros(0, 2 * d, device=dev())
    n, s = ops.rvq_code_stats(wide[:, d:], torch.zeros(0, dtype=torch.int64, device=dev()), C, torch.full((C,), SENTINEL, device=dev()),
                              torch.full((C, d), SENTINEL, device=dev()))
    assert n.shape == (C,) and s.shape == (C, d) and bool((n == 0).all()) and bool((s == 0).all())
