"""CPU: the causal flash-attention kernels (csrc/attention.hip) before any of them runs.  tests/attn_restated.py is proved against float64 autograd of the
dense formula; the inputs tests/test_gpu_attn_kernels.py hands the kernels are shown to execute what they are meant to (needle margins, the online
softmax's branches); the element-wise bounds are derived here, the rounded model is measured against them, and twelve wrong versions of the restatement
each miss one of them tenfold; the launchers' refusals run on the host.

BOUNDS.  Every bound is (a constant) x (the sum of the ABSOLUTE terms of that element), R.term_sums.  The constants come from the list of places where
the kernels round to bf16, never from a kernel's output.  One round-to-nearest to bf16 (8-bit significand) is at most U = 2^-8 relative -- reached just
above a power of two; the often quoted 2^-9 is the figure just below one -- so to first order, with T the term sum of the element:
  o     P (after the keep mask) is rounded before the second MFMA: U per term; O is rounded on store: U |o| <= U T.                      worst case 2 U T_o
  dv    P (after keep) is rounded before the dV MFMA; the partials and their sum stay fp32.                                              worst case 1 U T_dv
  dq    delta is computed from the STORED O: |d delta| <= U sum_d |dO O| = U tdelta, which enters dS as P tdelta; dS is rounded before the dQ MFMA:
        U |dS| <= U P (|dPt| + |delta|); dQ is rounded on store: U |dq|.  Each of the three is at most U T_dq with
        T_dq = scale sum_j P (|dPt| + tdelta) |k|.                                                                                        worst case 3 U T_dq
  dk    the same without the store (fp32 partials).                                                                                       worst case 2 U T_dk
  dtbl  takes the fp32 dS: only the rounded O inside delta, U scale sum P tdelta; plus the fp32 dot products (2^-16 of their absolute terms) and the
        block-scaled integers of the LDS window (each addend to 2^-19 of its pass's largest |dS|, bounded by the head's largest).         R.bounds
  lse   fp32 throughout: sim c2 - m, m / log2(e) and logf carry a few u32 of max |sim| (<= 60 nats: 3e-5).                                1e-4 + 8 u32 max|sim|
The kernels do not round where the model does: P is rounded un-normalised against a possibly stale maximum, sums run in another order, exp2 is the
hardware's.  Model and kernel are two draws under the same first-order worst case, so the BOUND IS TWICE THE WORST CASE (R.BOUND = 2 R.WORST; second-order
terms and fp32 summation, < 2^-15 relative, vanish in that factor), and the model has to stay at or below HALF of every bound -- which the derivation
guarantees if it is right; test_the_rounded_model_stays_under_half_of_every_bound measures it on every input of the GPU test and prints the ratios.
"""
import ctypes
import math
import os
import re

import pytest
import torch

import attn_restated as R
from audiolm_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('alm_mqa_attn_fwd', 'alm_mqa_attn_bwd', 'alm_mqa_attn_bias_fwd', 'alm_mqa_attn_bias_bwd', 'alm_attn_bias_part_rows', 'alm_attn_bias_grad_reduce',
           'alm_mqa_head_groups', 'alm_mqa_bwd_parts', 'alm_kv_grad_pack')
F64 = torch.float64
ALL = R.case_names() + R.variant_names()
OUTS = ('o', 'dq', 'dk', 'dv', 'dtbl')


def close(got, want, tol):
    return float((got - want).abs().max()) <= tol * max(1., float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize('name', [n for n in ALL if not n.startswith('needle') or n in ('needle-65-m', 'needle-200')])
def test_the_restatement_equals_float64_autograd_of_the_dense_formula(name):
    """softmax(scale (q k^T + bias) with hidden pairs at -finfo.max) keep / (1 - p) @ v through autograd, dead rows kept out of the loss (with that fill they
    are the uniform average, not this project's 0): o on the live rows, every gradient everywhere; the dead-row contract on its own"""
    c = R.case(name)
    ref, _, _ = R.reference(name)
    B, H, N, _ = c['q'].shape
    vis = R.visible(B, N, c['mask'])
    live = vis.any(-1)[:, 0]                                                                   # b n
    q, k, v = (c[x].clone().requires_grad_(True) for x in 'qkv')
    tbl = None
    S = torch.einsum('bhid,bjd->bhij', q, k)
    if c['tbl'] is not None:
        tbl = c['tbl'].clone().requires_grad_(True)
        S = S + torch.where((c['slot'] >= 0)[None], tbl[:, c['slot'].clamp(min=0)], torch.zeros((), dtype=F64))[None]
    A = (S * c['scale']).masked_fill(~vis, -torch.finfo(F64).max).softmax(-1)
    lse = torch.logsumexp((S.detach() * c['scale']).masked_fill(~vis, float('-inf')), -1)
    if c['keep'] is not None:
        A = A * c['keep'] / (1. - c['p'])
    o = torch.einsum('bhij,bjd->bhid', A, v)
    (o * c['dout'] * live[:, None, :, None]).sum().backward()
    lv = live[:, None, :, None].expand_as(o)
    assert close(ref['o'][lv], o.detach()[lv], 1e-12) and close(ref['lse'][live[:, None].expand(B, H, N)], lse[live[:, None].expand(B, H, N)], 1e-12)
    assert close(ref['dq'], q.grad, 1e-12) and close(ref['dk'], k.grad, 1e-12) and close(ref['dv'], v.grad, 1e-12)
    if tbl is not None:
        assert close(ref['dtbl'], tbl.grad, 1e-12) and float(ref['dtbl'].abs().max()) > 0
    # the contract for a query without a visible key, and for a key no live query sees
    dead = ~lv
    assert float(ref['o'][dead].abs().sum()) == 0. and float(ref['dq'][dead].abs().sum()) == 0. and bool((ref['lse'][~live[:, None].expand(B, H, N)] == float('-inf')).all())
    if c['mask'] is not None:
        assert float(ref['dk'][~c['mask']].abs().sum()) == 0. and float(ref['dv'][~c['mask']].abs().sum()) == 0.
    nd, nl = R.delta(ref['o'], c['dout'], ref['lse'], c['scale'])
    assert torch.equal(torch.isinf(nl), ~live[:, None].expand(B, H, N)) and bool((nl[torch.isinf(nl)] < 0).all()) and torch.equal(nd, -ref['delta'])


def test_the_prefix_case_has_every_dead_row_pattern():
    c = R.case('prefix')
    B, N = c['mask'].shape
    lengths = [int((~c['mask'][r]).sum()) for r in range(B)]
    assert lengths == [1, 31, 32, 33, 64, 65, N - 1, N, 0] and N == 129
    live = R.visible(B, N, c['mask']).any(-1)[:, 0]
    assert [int((~live[r]).sum()) for r in range(B)] == lengths                                # the first L queries of a row see no key


def test_the_dropout_hash_is_bernoulli_and_differs_between_heads_and_batch_rows():
    p, N = 0.25, 129
    keep = R.keep_mask(R.SEED, 2, 3, N, p)
    assert abs(float(keep.mean()) - (1 - p)) < 0.01
    assert float((keep[0, 0] == keep[0, 1]).double().mean()) < 0.7 and float((keep[0, 0] == keep[1, 0]).double().mean()) < 0.7
    # one pair by hand: the finaliser on plain Python integers
    salt = R.drop_salt(R.SEED, 1, 2, 3)
    x = (5 * N + 3) ^ salt
    for sh, mul in ((16, 0x7feb352d), (15, 0x846ca68b)):
        x ^= x >> sh
        x = (x * mul) & 0xffffffff
    x ^= x >> 16
    assert bool(keep[1, 2, 5, 3]) == (x >= R.drop_thr(p))


# ------------------------------------------------------------------------------------------------ what the inputs execute

@pytest.mark.parametrize('name', [n for n in R.case_names() if n.startswith('needle')])
def test_needles_are_one_hot_far_below_fp32_resolution(name):
    c = R.case(name)
    margin, off, dev64 = R.needle_margins(c)
    print(f'{name}: smallest margin {margin:.0f} nats, largest off-target mass {off:.1e}')
    assert margin >= 20. and off <= 1e-9 and dev64 == 0.
    ref, _, _ = R.reference(name)
    B, H, N, D = c['q'].shape
    live = c['target'] >= 0
    want = torch.gather(c['v'][:, None].expand(B, H, N, D), 2, c['target'].clamp(min=0)[..., None].expand(B, H, N, D))
    assert float((ref['o'] - want)[live].abs().max() if bool(live.any()) else 0.) <= 1e-12
    assert torch.equal(live, torch.isfinite(ref['lse']))
    assert float(ref['dq'].abs().max()) <= 1e-9 and float(ref['dk'].abs().max()) <= 1e-9         # dS = P (dP - delta) = 0: one key holds all the mass
    if N >= 129 and c['mask'] is None:
        assert bool((c['target'][:, 0, N - 1] == 64).all()) and (N < 200 or bool((c['target'][:, 0, N - 2] == 128).all()))


def test_needle_targets_cover_every_key_position_and_every_query_lane():
    """over the needle cases the targets hit every key position of a 64-key tile (key lane half x accumulator register) and come from every query lane
    (query mod 32); of the 32 x 64 (query lane, key position) pairs at least 95 % occur (the draw is random: 2001 of 2048)"""
    hit = torch.zeros(32, 64, dtype=torch.bool)
    for name in R.case_names():
        if name.startswith('needle'):
            t = R.case(name)['target']
            i = torch.arange(t.shape[2])[None, None].expand_as(t)
            hit[i[t >= 0] % 32, t[t >= 0] % 64] = True
    assert bool(hit.any(0).all()) and bool(hit.any(1).all()) and int(hit.sum()) >= 0.95 * 32 * 64


BRANCH = {'ramp-raise': 'raise', 'ramp-stale': 'defer', 'ramp-neg': 'keep'}


@pytest.mark.parametrize('name', list(BRANCH))
def test_every_ramp_takes_its_branch_of_the_online_softmax(name):
    """from the restated tile maxima (R.online_forward, which in exact arithmetic equals the plain softmax whatever it defers): 'raise' = the tile maximum
    exceeds m by more than 8 log2 units, 'defer' = it exceeds m by less and the wave does not rescale (P > 1 against a stale m), 'keep' = it does not"""
    c = R.case(name)
    a, _ = R.fwd_args(c)
    o, lse, census = R.online_forward(*a)
    ref, _, _ = R.reference(name)
    assert close(o, ref['o'], 1e-12) and close(lse, ref['lse'], 1e-12)
    print(name, census)
    B, H, N, _ = c['q'].shape
    first_tiles = B * H * N                                                                    # every row "raises" once, from -inf, on its first tile
    if name == 'ramp-raise':
        assert census['raise'] >= first_tiles + B * H * (N - 64) * 0.9                         # ... and here on (nearly) every later tile too
    if name == 'ramp-stale':
        assert census['defer'] >= B * H * 64 and census['raise'] > first_tiles                 # stale for whole tiles, then raised after all
    if name == 'ramp-neg':
        assert census['raise'] == first_tiles and census['defer'] == 0 and census['keep'] >= B * H * (N - 64)
    assert census[BRANCH[name]] > 0
    assert float(R.sim(c['q'], c['k'], c['scale']).abs().max()) <= 60.


def test_random_inputs_never_leave_the_first_tiles_maximum():
    """the gap this file's ramps close: with N(0, 1) inputs no row ever raises m after its first tile with a visible key"""
    for name in ('rand-1x257x8', 'rand-2x200x5-m'):
        c = R.case(name)
        B, H, N, _ = c['q'].shape
        _, _, census = R.online_forward(*R.fwd_args(c)[0])
        assert census['raise'] == int(R.visible(B, N, c['mask']).any(-1).sum()) * H


# ------------------------------------------------------------------------------------------------ bounds

@pytest.mark.parametrize('name', ALL)
def test_the_rounded_model_stays_under_half_of_every_bound(name):
    ref, T, bound = R.reference(name)
    model = R.model(name)
    outs = [n for n in OUTS if n in ref]
    rs = {n: R.ratio(model[n], ref[n], bound[n]) for n in outs}
    print(f'{name:28s} model error / bound: ' + '  '.join(f'{n} {rs[n]:.3f}' for n in outs))
    for n in outs:
        assert rs[n] <= 0.5, (name, n, rs[n])
        assert bool((T[n] * (1 + 1e-12) + 1e-300 >= ref[n].abs()).all()) or n == 'dtbl', (name, n)       # a sum of absolute terms dominates the element
    assert torch.equal(model['lse'], ref['lse'])                                                         # no bf16 point touches the statistic
    assert float(bound['lse'].max()) <= 1e-4 + 64 * 8 * 2.0 ** -24                                        # |sim| <= 60 nats, the needles' 64


def test_the_constants_are_the_derivations():
    assert R.U == 2.0 ** -8 and R.WORST == dict(o=2 * R.U, dq=3 * R.U, dk=2 * R.U, dv=R.U, dtbl=R.U) and all(R.BOUND[n] == 2 * R.WORST[n] for n in R.WORST)
    x = torch.tensor([1. + 2.0 ** -8 + 2.0 ** -20], dtype=F64)                                           # just above a power of two: the rounding's worst case
    assert 0.99 * R.U <= float((R.bf(x) - x).abs() / x) <= R.U


# ------------------------------------------------------------------------------------------------ mutants of the restatement

def _with(monkeypatch, name, visible=None, **over):
    """reference-style outputs of case `name` with R.visible replaced and / or inputs overridden"""
    c = dict(R.case(name), **over)
    if visible is not None:
        monkeypatch.setattr(R, 'visible', visible)
    a, kw = R.fwd_args(c)
    o, lse, _ = R.attention(*a, **kw)
    out = R.backward(*a, c['dout'], **kw, o=o, lse=lse, slot=c['slot'], LT=c['LT'])
    out.update(o=o, lse=lse)
    monkeypatch.undo()
    return out


_vis = R.visible


def _causal_ge(B, N, mask):
    return _vis(B, N, mask) & ~torch.eye(N, dtype=torch.bool)


def _tile_key_lost(B, N, mask):
    v = _vis(B, N, mask).clone()
    for j in range(64, N, 64):
        v[:, :, j + 1:, j] = False
    return v


def _one_key_unmasked(B, N, mask):
    m = mask.clone()
    for b in range(B):
        hid = (~m[b]).nonzero()
        if len(hid):
            m[b, int(hid[0])] = True
    return _vis(B, N, m)


def _mask_of_batch_0(B, N, mask):
    m = mask.clone()
    m[1] = m[0]
    return _vis(B, N, m)


def m_causal_ge(mp, n):
    return _with(mp, n, _causal_ge)


def m_tile_key_lost(mp, n):
    return _with(mp, n, _tile_key_lost)


def m_one_key_unmasked(mp, n):
    return _with(mp, n, _one_key_unmasked)


def m_mask_of_batch_0(mp, n):
    return _with(mp, n, _mask_of_batch_0)


def m_delta_of_the_next_head(mp, n):
    c, (ref, _, _) = R.case(n), R.reference(n)
    a, kw = R.fwd_args(c)
    out = R.backward(*a, c['dout'], **kw, o=ref['o'], lse=ref['lse'], delta_=ref['delta'].roll(1, 1))
    return dict(ref, dq=out['dq'], dk=out['dk'])


def m_dk_without_scale(mp, n):
    ref = R.reference(n)[0]
    return dict(ref, dk=ref['dk'] / R.case(n)['scale'])


def m_lse_off_by_log2(mp, n):
    ref = R.reference(n)[0]
    return dict(ref, lse=ref['lse'] + math.log(2.))


def m_rescale_skipped(mp, n):
    o, lse, _ = R.online_forward(*R.fwd_args(R.case(n))[0], skip_rescale=True)
    return dict(R.reference(n)[0], o=o, lse=lse)


def m_dead_rows_uniform(mp, n):
    c, ref = R.case(n), R.reference(n)[0]
    dead = torch.isinf(ref['lse'])[..., None]
    return dict(ref, o=torch.where(dead, c['v'].mean(1)[:, None, None, :], ref['o']))


def m_dropped_pair_in_dv(mp, n):
    c, ref = R.case(n), R.reference(n)[0]
    a, kw = R.fwd_args(c)
    P = R.attention(*a, **kw)[2]
    return dict(ref, dv=torch.einsum('bhij,bhid->bjd', P, c['dout']) / (1. - c['p']))


def m_keep_of_the_previous_head(mp, n):
    return _with(mp, n, keep=R.case(n)['keep'].roll(1, 1))


# mutant -> (the GPU-test input that catches it, the output whose bound it misses)
MUTANTS = {m_causal_ge: ('needle-129', 'o'), m_tile_key_lost: ('needle-200', 'o'), m_one_key_unmasked: ('prefix', 'o'), m_mask_of_batch_0: ('prefix', 'o'),
           m_delta_of_the_next_head: ('needle-200-m', 'dq'), m_dk_without_scale: ('rand-2x96x4-m', 'dk'), m_lse_off_by_log2: ('rand-1x63x8', 'lse'),
           m_rescale_skipped: ('ramp-raise', 'o'), m_dead_rows_uniform: ('prefix', 'o'), m_dropped_pair_in_dv: ('prefix+nobias+p0.25', 'dv'),
           m_keep_of_the_previous_head: ('ramp-raise+nobias+p0.25', 'o')}


@pytest.mark.parametrize('mutant', list(MUTANTS), ids=lambda f: f.__name__[2:])
def test_each_mutant_of_the_restatement_misses_a_bound_tenfold(mutant, monkeypatch):
    name, out = MUTANTS[mutant]
    assert name in ALL
    ref, _, bound = R.reference(name)
    got = mutant(monkeypatch, name)
    r = R.ratio(got[out], ref[out], bound[out])
    print(f'{mutant.__name__[2:]:28s} on {name:26s} {out}: error / bound {r:.1f}')
    assert r >= 10., (mutant.__name__, name, out, r)
    assert R.visible is _vis


def test_the_delta_mutant_really_takes_the_neighbours_delta():
    c, ref = R.case('needle-200-m'), R.reference('needle-200-m')[0]
    assert c['q'].shape[1] >= 3
    d = R.delta(ref['o'], c['dout'], ref['lse'], c['scale'])[0]
    assert float((d - d.roll(1, 1)).abs().max()) > 1.


def kv_parts(nparts, rows, seed):
    g = R.gen(seed)
    return torch.randn(nparts, rows, 2 * R.DH, generator=g).float().double(), torch.randn(rows, R.DH, generator=g).float().double()


def kv_pack_bound(parts, acc, mode):
    """the float64 sum rounded ONCE to bf16 (worst case U of the result) after fp32 additions (2^-20 of the absolute terms); the bound is twice the worst
    case, as everywhere in this file"""
    want, acc2 = R.kv_grad_pack(parts, acc, mode)
    terms, _ = R.kv_grad_pack(parts.abs(), acc.abs(), mode)
    return want, acc2, 2 * (R.U * want.abs() + 2.0 ** -20 * terms)


@pytest.mark.parametrize('nparts', [2, 4])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_a_partial_set_left_out_of_kv_grad_pack_misses_its_bound_tenfold(nparts, mode):
    parts, acc = kv_parts(nparts, 77, 5 + nparts)
    want, _, bound = kv_pack_bound(parts, acc, mode)
    got, _ = R.kv_grad_pack(parts, acc, mode, skip=1)
    assert R.ratio(got, want, bound) >= 10. and R.ratio(R.bf(want), want, bound) <= 0.5 + 1e-9


# ------------------------------------------------------------------------------------------------ the C ABI on the host

def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} is not declared in include/audiolm_hip.h'
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(',')), name
        assert hasattr(lib, name), name
    assert 'attention.hip' in __import__('audiolm_pytorch_amd.build', fromlist=['SOURCES']).SOURCES
    assert _lib.query('alm_mqa_bwd_parts', 2, 5, 3) == 1 and _lib.query('alm_mqa_bwd_parts', 2, 5, 8) == 2 and _lib.query('alm_mqa_bwd_parts', 1, 129, 3) == 2


def test_the_launchers_refuse_on_the_host():
    """every entry point checks its arguments before the launch: the refusal comes back on a machine without a GPU.  X is a non-null, 16-byte aligned address
    that is never dereferenced (each call below has exactly one defect and is refused for it)."""
    q, BAD, UNS, X = _lib.query, 10001, 10002, ctypes.c_void_p(4096)
    assert os.environ.get('ALM_ATTN_DKV_NH') is None and os.environ.get('ALM_ATTN_DKV_SPLIT') is None

    def each(name, good, defects, code=BAD):
        for i, v in defects:
            args = list(good)
            args[i] = v
            assert q(name, *args) == code, (name, i, v)

    B, N, H = 2, 5, 3                                      # H * 64 = 192
    # q, ldq, k, ldk, v, ldv, mask, o, ldo, lse, B, N, H, dim_head, scale, dropout_p, seed, seed_dev, stream
    fwd = [X, 200, X, 72, X, 72, None, X, 196, X, B, N, H, 64, 0.125, 0., 0, None, None]
    fwd_defects = [(0, None), (2, None), (4, None), (7, None), (9, None), (1, 184), (8, 188), (3, 56), (5, 56), (1, 196), (8, 194), (15, 1.0)]
    each('alm_mqa_attn_fwd', fwd, fwd_defects)
    each('alm_mqa_attn_fwd', fwd, [(10, 0), (11, 0), (12, 0), (12, 65), (13, 32)], UNS)
    tail = [X, 2 * N, X, X, X, X]                          # tbl, LT, qkey4, kkey4, qattr, kattr
    each('alm_mqa_attn_bias_fwd', fwd[:15] + tail + fwd[15:], fwd_defects[:11] + [(15, None), (17, None), (16, 1)])
    # q, ldq, k, ldk, v, ldv, mask, o, ldo, lse, dout, lddo, dq, lddq, dk, dv, lddk, part_stride, delta, B, N, H, dim_head, scale, dropout_p, seed, seed_dev, stream
    bwd = [X, 200, X, 72, X, 72, None, X, 196, X, X, 200, X, 196, X, X, 136, 0, X, B, N, H, 64, 0.125, 0., 0, None, None]
    bwd_defects = [(i, None) for i in (0, 2, 4, 7, 9, 10, 12, 14, 15, 18)] + [(1, 184), (8, 188), (11, 184), (13, 188), (3, 56), (5, 56), (16, 56), (11, 196), (13, 194)]
    each('alm_mqa_attn_bwd', bwd, bwd_defects)
    each('alm_mqa_attn_bwd', bwd, [(19, 0), (20, 0), (21, 0), (22, 32)], UNS)
    each('alm_mqa_attn_bias_bwd', bwd[:24] + tail + [X] + bwd[24:], bwd_defects + [(24, None), (30, None)])
    # two partial sets (H = 8): the second must not start inside the first
    H8 = list(bwd)
    H8[1], H8[8], H8[11], H8[13], H8[21] = 520, 516, 520, 516, 8
    assert q('alm_mqa_bwd_parts', B, N, 8) == 2
    each('alm_mqa_attn_bwd', H8, [(17, 0), (17, B * N * 136 - 8), (17, -1)])
    # dk, dv, ld, nparts, part_stride, acc_v0, dkv_bf16, ldo, rows, dim_head, mode, stream
    pack = [X, X, 136, 2, 10 * 136, None, X, 136, 10, 64, 0, None]
    each('alm_kv_grad_pack', pack, [(0, None), (1, None), (6, None), (2, 56), (7, 120), (4, 10 * 136 - 8), (3, 0), (10, 3), (10, 1), (9, 0), (8, -1)])
    assert q('alm_kv_grad_pack', None, None, 0, 1, 0, None, None, 0, 0, 64, 0, None) == 0          # no rows: nothing to do
