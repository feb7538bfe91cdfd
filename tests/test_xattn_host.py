"""CPU: the conditioning-attention path (audiolm_pytorch_amd/xattn.py, csrc/xattn.hip) before any kernel runs.  The float64 restatement
(tests/xattn_restated.py) is checked against the oracle's Attend on the concatenated key set; the merged form (self part, then the extra keys through the
joint log-sum-exp, then the combine) and the backward pieces (delta of the JOINT output, dS, dbias) are proved equal to one softmax over all keys, which is
what tests/test_gpu_xattn.py leans on; the launchers' refusals run on the host; the five symbols are declared, bound and exported."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import audiolm_oracle as O
import xattn_restated as R
from audiolm_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('alm_xattn_softmax_fwd', 'alm_xattn_combine', 'alm_xattn_softmax_bwd', 'alm_xattn_delta', 'alm_xattn_dbias')
F64 = torch.float64

# the small shapes of the GPU composition tests
CASES = {'cross-Me1': lambda: R.cross_case(2, 37, 3, 1, 64), 'cross-N1': lambda: R.cross_case(1, 1, 8, 7, 64), 'cross-Me130': lambda: R.cross_case(3, 33, 6, 130, 64),
         'prefix-m5': lambda: R.prefix_case(2, 37, 8, 5, 64), 'prefix-m64': lambda: R.prefix_case(1, 130, 4, 64, 64),
         'dense-causal': lambda: R.dense_case('causal'), 'dense-causal-prefix': lambda: R.dense_case('causal_prefix'), 'dense-noncausal': lambda: R.dense_case('noncausal')}


def close(got, want, tol):
    return float((got - want).abs().max()) <= tol * max(1., float(want.abs().max()))


def rows(t):
    """(b h n x) -> the kernels' [B, N, H, x]"""
    return t.permute(0, 2, 1, 3)


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('p', [0., 0.25])
def test_joint_attention_equals_the_oracle_on_the_concatenated_keys(name, p):
    """every row of these cases keeps at least one visible key (the oracle's -finfo.max fill would make a fully hidden row uniform: not the library's contract)"""
    c = CASES[name]()
    B, H, N, dh = c['q'].shape
    ks = [t for t in (c['ke'], c['k_self']) if t is not None]
    keep = (torch.rand(B, H, N, sum(t.shape[1] for t in ks), generator=torch.Generator().manual_seed(5)) >= p).double() if p else None
    ref = R.reference(c, keep=keep, p=p)
    vs = [t for t in (c['ve'], c['v_self']) if t is not None]
    ones = lambda n: torch.ones(B, n, dtype=torch.bool)
    masks = []
    if c['ke'] is not None:
        masks.append(ones(c['ke'].shape[1]) if c['emask'] is None else c['emask'])
    if c['k_self'] is not None:
        masks.append(ones(N) if c['self_mask'] is None else c['self_mask'])
    mask = torch.cat(masks, 1)
    assert bool(mask.any(1).all())
    q = c['q'].clone().requires_grad_(True)
    k, v = torch.cat(ks, 1).clone().requires_grad_(True), torch.cat(vs, 1).clone().requires_grad_(True)
    bias = None if c['bias'] is None else c['bias'].clone().requires_grad_(True)
    if name == 'dense-causal-prefix':
        assert float(c['bias'][:, :, :5].abs().max()) == 0. and torch.equal(c['bias'], F.pad(c['bias'][:, :, 5:], (5, 0), value=0.))     # audiolm_pytorch.py:345
    out = O.attend(q, k, v, mask=mask, attn_bias=bias, causal=c['k_self'] is not None, keep=keep, p_drop=p)
    assert out.dtype == F64
    out.backward(c['dout'])
    Me = 0 if c['ke'] is None else c['ke'].shape[1]
    assert close(ref['o'], out.detach(), 1e-12)
    assert close(ref['dq'], q.grad, 1e-12)
    for part, sl in (('dke', slice(0, Me)), ('dk_self', slice(Me, None))):
        if ref[part] is not None:
            assert close(ref[part], k.grad[:, sl], 1e-12), part
    for part, sl in (('dve', slice(0, Me)), ('dv_self', slice(Me, None))):
        if ref[part] is not None:
            assert close(ref[part], v.grad[:, sl], 1e-12), part
    if bias is not None:
        assert close(ref['dbias'], bias.grad, 1e-12)


@pytest.mark.parametrize('name', list(CASES))
def test_the_merged_form_equals_joint_attention(name):
    """self part alone -> softmax_part with that lse_self -> combine; the dense cases put every key through softmax_part with the causal offset Me - N"""
    c = CASES[name]()
    B, H, N, dh = c['q'].shape
    want, want_lse = R.joint_attention(*R.attention_args(c), bias=c['bias'], return_lse=True)
    if c['flash_self']:
        o_self = lse_self = None
        if c['k_self'] is not None:
            o_self, lse_self = R.joint_attention(c['q'], c['k_self'], c['v_self'], c['self_mask'], None, None, None, c['scale'], return_lse=True)
        ke, ve, emask, bias, off = c['ke'], c['ve'], c['emask'], None, R.NOT_CAUSAL
    else:
        o_self = lse_self = None
        ke = torch.cat([t for t in (c['ke'], c['k_self']) if t is not None], 1)
        ve = torch.cat([t for t in (c['ve'], c['v_self']) if t is not None], 1)
        bias = c['bias']
        off = ke.shape[1] - N if c['k_self'] is not None else R.NOT_CAUSAL
        emask = None
        if c['k_self'] is not None:
            pm = torch.ones(B, ke.shape[1] - N, dtype=torch.bool) if c['emask'] is None else c['emask']
            emask = torch.cat((pm, c['self_mask']), 1)
        else:
            emask = c['emask']
    S = rows(torch.einsum('bhid,bjd->bhij', c['q'], ke))
    P, lse, fself = R.softmax_part(S, c['scale'], emask, lse_self, bias, off)
    o_e = torch.einsum('bnhj,bjd->bnhd', P, ve)
    o = R.combine(None if o_self is None else rows(o_self), fself, o_e)
    assert close(rows(o), want, 1e-12) and close(lse, want_lse, 1e-12)
    if lse_self is None:
        assert float(fself.abs().max()) == 0.
    elif B > 1:                                                       # the batch row whose whole prefix is masked: the self part alone, exactly
        assert torch.equal(lse[B - 1], lse_self[B - 1]) and torch.equal(rows(o)[B - 1], o_self[B - 1]) and bool((fself[B - 1] == 1).all())


@pytest.mark.parametrize('name,p', [(n, 0.) for n in CASES] + [(n, 0.25) for n in CASES if not n.startswith('prefix')])     # flash dropout: test_gpu_dropout.py
def test_the_backward_pieces_equal_autograd_of_joint_attention(name, p):
    """delta on the JOINT output, then dS = P o (dP + ndelta) * scale per key set (each set's P normalised by the joint lse), dbias = sum_b of the
    un-scaled dS: dq, dk, dv and dbias equal autograd through one softmax over all keys, with and without a keep mask on the xattn key set"""
    c = CASES[name]()
    B, H, N, dh = c['q'].shape
    keep = R.keep_for(c, p) if p else None
    ref, _ = R.model_and_reference(c, keep=keep, p=p)
    do, q = rows(c['dout']), rows(c['q'])
    nd = R.delta(rows(ref['o']), do)
    flash = c['flash_self'] and c['k_self'] is not None
    if c['flash_self']:
        kx, vx, mx, bias, off = c['ke'], c['ve'], c['emask'], None, R.NOT_CAUSAL
    else:
        kx = torch.cat([t for t in (c['ke'], c['k_self']) if t is not None], 1)
        vx = torch.cat([t for t in (c['ve'], c['v_self']) if t is not None], 1)
        bias = c['bias']
        off = kx.shape[1] - N if c['k_self'] is not None else R.NOT_CAUSAL
        mx = c['emask']
        if c['k_self'] is not None:
            mx = torch.cat((torch.ones(B, kx.shape[1] - N, dtype=torch.bool) if c['emask'] is None else c['emask'], c['self_mask']), 1)
    Sx = torch.einsum('bnhd,bjd->bnhj', q, kx)
    lse_other = None
    if flash:                                                         # each part sees the other one only through its log-sum-exp
        Ss = torch.einsum('bnhd,bjd->bnhj', q, c['k_self'])
        _, lse_other, _ = R.softmax_part(Ss, c['scale'], c['self_mask'], None, None, 0)
    P, lse, _ = R.softmax_part(Sx, c['scale'], mx, lse_other, bias, off)
    assert close(lse, ref['lse'], 1e-12)
    kp = None if keep is None else rows(keep)
    da = 1. / (1. - p)
    Pd = P if kp is None else P * kp
    dP = torch.einsum('bnhd,bjd->bnhj', do, vx) * (1. if kp is None else da * kp)
    dS = R.softmax_bwd(P, dP, nd, c['scale'])
    dq = torch.einsum('bnhj,bjd->bnhd', dS, kx)
    dkx, dvx = torch.einsum('bnhj,bnhd->bjd', dS, q), torch.einsum('bnhj,bnhd->bjd', Pd, do) * (1. if kp is None else da)
    if flash:
        _, lse_x, _ = R.softmax_part(Sx, c['scale'], mx, None, None, R.NOT_CAUSAL)
        Pf, lse2, _ = R.softmax_part(Ss, c['scale'], c['self_mask'], lse_x, None, 0)
        assert close(lse2, ref['lse'], 1e-12)
        dSf = R.softmax_bwd(Pf, torch.einsum('bnhd,bjd->bnhj', do, c['v_self']), nd, c['scale'])
        dq = dq + torch.einsum('bnhj,bjd->bnhd', dSf, c['k_self'])
        assert close(torch.einsum('bnhj,bnhd->bjd', dSf, q), ref['dk_self'], 1e-10) and close(torch.einsum('bnhj,bnhd->bjd', Pf, do), ref['dv_self'], 1e-10)
    Me = 0 if c['ke'] is None else c['ke'].shape[1]
    assert close(rows(dq), ref['dq'], 1e-10)
    if c['ke'] is not None:
        assert close(dkx[:, :Me], ref['dke'], 1e-10) and close(dvx[:, :Me], ref['dve'], 1e-10)
    if not c['flash_self'] and c['k_self'] is not None:
        assert close(dkx[:, Me:], ref['dk_self'], 1e-10) and close(dvx[:, Me:], ref['dv_self'], 1e-10)
    if bias is not None:
        assert close(R.dbias(P, dP, nd), ref['dbias'], 1e-10)


def test_the_rounded_model_stays_under_the_flash_tests_ceiling():
    """the bound of the GPU composition tests is twice the model's error, capped by the flash kernels' own bounds (5e-3 / 3e-3 forward, 1e-2 / 4e-3
    backward, rel-max / rel-Frobenius): a model that is itself above that ceiling is mis-stated"""
    for name, make in CASES.items():
        c = make()
        ref, model = R.model_and_reference(c)
        mags = R.term_magnitudes(c)
        for k, (cm, cf) in dict(o=(5e-3, 3e-3), dq=(1e-2, 4e-3), dke=(1e-2, 4e-3), dve=(1e-2, 4e-3), dk_self=(1e-2, 4e-3), dv_self=(1e-2, 4e-3), dbias=(1e-2, 4e-3)).items():
            if ref[k] is None:
                continue
            if name == 'cross-Me1' and k != 'dq':       # one key: P = 1 exactly, so o = v_e and dv_e = sum dO with no rounding, and dS = P (dP - delta) = 0
                assert float((model[k] - ref[k]).abs().max()) <= 1e-12 and (k != 'dke' or float(ref[k].abs().max()) <= 1e-12), k
                continue
            em, ef = R.relmax(model[k], ref[k]), R.relfrob(model[k], ref[k])
            print(f'{name:20s} {k:8s} model rel-max {em:.2e} rel-frob {ef:.2e}')
            if name == 'cross-Me1':                    # dq = 0 up to float64 noise: no relative error to speak of
                continue
            assert 0. < em <= cm and 0. < ef <= cf, (name, k, em, ef)
            assert bool((mags[k] >= ref[k].abs() * (1 - 1e-12)).all()), (name, k)
        assert torch.equal(model['lse'], ref['lse'])                    # no rounding point touches the statistic


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} is not declared in include/audiolm_hip.h'
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(',')), name
        assert hasattr(lib, name), name
    assert 'xattn.hip' in __import__('audiolm_pytorch_amd.build', fromlist=['SOURCES']).SOURCES


def test_the_launchers_refuse_on_the_host():
    """every entry point checks its arguments before the launch: ALM_ERR_BAD_ARG comes back on a machine without a GPU.  X is a non-null address that is
    never dereferenced (each call below has exactly one defect and is refused for it)."""
    q, BAD, X = _lib.query, 10001, ctypes.c_void_p(4096)
    NC = 0x7fffffff

    def each(name, good, defects):
        for i, v in defects:
            args = list(good)
            args[i] = v
            assert q(name, *args) == BAD, (name, i, v)

    # S, ldS, emask, lse_self, scale, P, ldP, lse_tot, fself, bias, ldbias, causal_off, B, N, H, Me, stream
    each('alm_xattn_softmax_fwd', [X, 16, None, None, 1.0, X, 16, X, None, None, 0, NC, 2, 5, 3, 9, None],
         [(0, None), (5, None), (7, None), (12, 0), (13, 0), (14, 0), (15, 0), (12, -1), (1, 8), (6, 8)])
    assert q('alm_xattn_softmax_fwd', X, 16, None, None, 1.0, X, 16, X, None, X, 8, NC, 2, 5, 3, 9, None) == BAD           # a bias narrower than Me
    # o_self, ldos, fself, o_e, out, ldo, tokens, H, dim_head, stream
    each('alm_xattn_combine', [None, 0, None, X, X, 96, 10, 3, 32, None], [(3, None), (4, None), (6, 0), (7, 0), (8, 0), (8, 30), (5, 92), (5, 64)])
    each('alm_xattn_combine', [X, 96, X, X, X, 96, 10, 3, 32, None], [(2, None), (1, 64), (1, 98)])
    # P, ldP, dP, lddP, ndelta, scale, dS, lddS, Me, B, N, H, stream
    each('alm_xattn_softmax_bwd', [X, 16, X, 16, X, 1.0, X, 24, 9, 2, 5, 3, None],
         [(0, None), (2, None), (4, None), (6, None), (8, 0), (9, 0), (10, 0), (11, 0), (1, 8), (3, 8), (7, 8)])
    # o, ldo, dout, lddo, ndelta, B, N, H, dim_head, stream
    each('alm_xattn_delta', [X, 200, X, 192, X, 2, 5, 3, 64, None], [(0, None), (2, None), (4, None), (5, 0), (6, 0), (7, 0), (8, 0), (8, -64), (1, 191), (3, 191)])
    # P, ldP, dP, lddP, ndelta, dbias, lddb, Me, B, N, H, stream
    each('alm_xattn_dbias', [X, 16, X, 16, X, X, 14, 9, 2, 5, 3, None],
         [(0, None), (2, None), (4, None), (5, None), (7, 0), (8, 0), (9, 0), (10, 0), (1, 8), (3, 8), (6, 8)])
