"""Conditioning attention (csrc/xattn.hip, audiolm_pytorch_amd/xattn.py) on a real MI355X, against the float64 restatement tests/xattn_restated.py.

a. One test per C-ABI entry point, called through _lib.call on inputs built here: every branch of the kernels' header comments (mask or none, self part or
   none, bias or none, each causal_off regime, a padded leading dimension on every operand that has one), memory the kernels must not read poisoned with
   NaN, outputs pre-filled with NaN, guards after the last row / column; and one case per kernel with more rows than one pass of the 16384-workgroup grid.
b. The compositions xattn.extra_attn_fwd / extra_attn_bwd -- cross-attention, the prefix merged into the flash kernels' result through the joint
   log-sum-exp, the dense-bias math path, and the drawn dropout mask -- against ONE softmax over the concatenated key set (joint_attention).

Bounds.  bf16 outputs of the single kernels: one round-to-nearest-even is 2^-9 relative, the bound is 2^-8 of the magnitude of the TERMS, element-wise
(__expf and the fp32 operation order contribute ~|x| 1e-7, |x| <= 40).  fp32 outputs: 1e-4 (absolute for lse, |lse| <= 30; relative to the sum of absolute
terms for the others) -- expected ~1e-6.  Compositions: twice the error of rounded_model against joint_attention on the same inputs (both on the reference
side), capped by the flash test's own bounds (5e-3 / 3e-3 forward, 1e-2 / 4e-3 backward, rel-max / rel-Frobenius); see `compare`.  At these small shapes a
query sees a handful of keys, the roundings do not average out and twice the model often exceeds that cap: the cap is then the bound, the tighter of the two
(the model itself stays under it: tests/test_xattn_host.py, which also proves the restated formulas on the CPU)."""
import functools

import pytest
import torch

import xattn_restated as R

pytestmark = pytest.mark.gpu

BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
NOT_CAUSAL = 0x7fffffff
NAN = float('nan')
EPS = 2.0 ** -8
SCALE = 0.125


@pytest.fixture(scope='module')
def lib():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import _lib, ops, xattn
    return type('Lib', (), dict(call=staticmethod(_lib.call), ops=ops, xattn=xattn, st=staticmethod(ops._st)))


def dev():
    return torch.device('cuda:0')


def gen(seed):
    return torch.Generator().manual_seed(seed)


def uni(g, *shape, lo=-1., hi=1.):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def pad8(n):
    return (n + 7) // 8 * 8


def nan_buf(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def all_nan(t):
    return bool(torch.isnan(t).all())


SHAPES = [(2, 37, 3, 1), (1, 1, 8, 7), (2, 50, 8, 64), (2, 50, 6, 65), (3, 33, 5, 130)]        # (B, N, H, Me)
GRID_STRIDE = (1, 8200, 8, 9)                                                                 # 65600 rows > 16384 workgroups x 4 rows


# ------------------------------------------------------------------------------------------------ a. alm_xattn_softmax_fwd

def softmax_fwd_case(lib, B, N, H, Me, ld_extra, use_mask, use_lse, use_bias, causal_off, want_fself):
    g = gen(B * 1000 + N * 7 + H * 3 + Me + (causal_off & 0xff))
    rows, ldP = B * N * H, pad8(Me)
    ldS, ldb = ldP + ld_extra, Me + 3
    off = R.NOT_CAUSAL if causal_off == NOT_CAUSAL else causal_off
    emask = R.extra_mask(B, Me, g) if use_mask else None
    vis = R._visible(B, N, Me, emask, off, 'cpu').expand(B, N, H, Me)
    S = torch.full((B, N, H, ldS), NAN)
    S[..., :Me] = torch.where(vis, uni(g, B, N, H, Me, lo=-12., hi=12.) / SCALE, torch.tensor(NAN))     # scores span +-12 after scaling; hidden ones are poison
    bias = None
    if use_bias:
        bias = torch.full((H, N, ldb), NAN)
        causal_vis = R._visible(1, N, Me, None, off, 'cpu')[0, :, 0]                                    # [N, Me]: hidden for EVERY batch row
        bias[..., :Me] = torch.where(causal_vis[None], uni(g, H, N, Me, lo=-2., hi=2.), torch.tensor(NAN))
    S, bias = S.to(dev()), None if bias is None else bias.to(dev())
    emask_d = None if emask is None else emask.to(dev())
    S64, bias64 = S[..., :Me].double(), None if bias is None else bias[..., :Me].double()
    lse_self = None
    if use_lse:          # spread over +-15 around the extra part's lse: fself -> 0 and fself -> 1 both occur; rows with no visible key get a finite value too
        _, lse_e, _ = R.softmax_part(S64, SCALE, emask_d, None, bias64, off)
        lse_self = (torch.where(torch.isinf(lse_e), torch.zeros_like(lse_e), lse_e) + uni(g, B, H, N, lo=-15., hi=15.).to(dev()).double()).float().contiguous()
    wantP, want_lse, want_f = R.softmax_part(S64, SCALE, emask_d, None if lse_self is None else lse_self.double(), bias64, off)
    P = nan_buf((rows + 1, ldP), BF16)                                                                 # + one guard row
    lse = nan_buf((B, H, N), F32)
    fself = nan_buf((rows,), F32) if want_fself else None
    mu8 = None if emask is None else emask_d.to(U8).contiguous()
    lib.call('alm_xattn_softmax_fwd', S.data_ptr(), ldS, lib.ops._p(mu8), lib.ops._p(lse_self), SCALE, P.data_ptr(), ldP, lse.data_ptr(), lib.ops._p(fself),
             lib.ops._p(bias), ldb if use_bias else 0, causal_off, B, N, H, Me, lib.st())
    torch.cuda.synchronize()
    tag = (B, N, H, Me, ld_extra, use_mask, use_lse, use_bias, causal_off)
    assert all_nan(P[rows]), ('guard row of P written', tag)
    got = P[:rows].double().view(B, N, H, ldP)
    vis_d = vis.to(dev())
    assert not bool(torch.isnan(got).any()), ('P holds NaN: a hidden or pad position was read, or a column was not written', tag)
    assert float(got[..., Me:].abs().sum()) == 0. and float(got[..., :Me][~vis_d].abs().sum()) == 0., ('P not 0 in a hidden / pad column', tag)
    errP = (got[..., :Me] - wantP).abs() - (EPS * wantP + 1e-6)
    assert float(errP.max()) <= 0., ('P', tag, float(errP.max()))                                    # observed on MI355X: max |err| / (2^-8 P + 1e-6) <= 0.996
    fin = torch.isfinite(want_lse)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float('-inf')).all()), ('lse -inf pattern', tag)
    e_lse = float((lse.double() - want_lse)[fin].abs().max()) if bool(fin.any()) else 0.
    assert e_lse <= 1e-4, ('lse_tot', tag, e_lse)
    none_vis = ~vis_d.any(-1)                                                                          # [B, N, H]: rows with no visible extra key
    stats = dict(P=float(((got[..., :Me] - wantP).abs() / (EPS * wantP + 1e-6)).max()), lse=e_lse, fself=0.)
    if lse_self is not None and bool(none_vis.any()):
        nv = none_vis.permute(0, 2, 1)
        assert torch.equal(lse[nv], lse_self[nv]), ('lse_tot != lse_self bit for bit in a row without a visible extra key', tag)
    if fself is not None:
        f = fself.double().view(B, N, H)
        rel = (f - want_f).abs() / (want_f + 1e-12)
        assert float(rel.max()) <= 1e-4, ('fself', tag, float(rel.max()))
        stats['fself'] = float(rel.max())
        if lse_self is not None:
            assert bool((f[none_vis] == 1.).all()), ('fself != 1 in a row without a visible extra key', tag)
            assert rows < 1000 or (float(f.min()) < 1e-3 and float(f.max()) > 1 - 1e-3)                # both ends of the merge occur
        else:
            assert float(f.abs().sum()) == 0., ('fself != 0 without a self part', tag)
    if lse_self is None and bool(none_vis.any()):
        assert float(got[none_vis].abs().sum()) == 0. and bool((lse[none_vis.permute(0, 2, 1)] == float('-inf')).all()), ('dead row', tag)
    return stats


def run_softmax_fwd_matrix(lib, B, N, H, Me, ld_extra, causal_off):
    worst = dict(P=0., lse=0., fself=0.)
    for use_mask in (False, True):
        for use_lse in (False, True):
            for use_bias in (False, True):
                s = softmax_fwd_case(lib, B, N, H, Me, ld_extra, use_mask, use_lse, use_bias, causal_off, want_fself=use_lse or use_mask)
                worst = {k: max(worst[k], s[k]) for k in worst}
    print(f'softmax_fwd {(B, N, H, Me)} ldS-ldP={ld_extra} causal_off={causal_off}: P err / bound {worst["P"]:.3f}, lse abs {worst["lse"]:.2e}, fself rel {worst["fself"]:.2e}')


@pytest.mark.parametrize('causal_off', [NOT_CAUSAL, 0, 5, -5])
@pytest.mark.parametrize('B,N,H,Me,ld_extra', [(*s, 0) for s in SHAPES] + [(2, 50, 6, 65, 8)])
def test_softmax_fwd(lib, B, N, H, Me, ld_extra, causal_off):
    """{no mask, emask} x {no self part, lse_self} x {no bias, bias with ldbias = Me + 3} per shape and causal regime (causal_off = -5: the first queries see no
    key).  Observed on MI355X over all cases: P at most 0.996 of its bound (one correct rounding reaches 2^-8 / (1 + 2^-8) = 0.9961 of it: the bound is the
    worst case of ONE rounding, a second half-ulp does not fit), lse_tot <= 1.5e-6 absolute, fself <= 2.4e-6 relative"""
    run_softmax_fwd_matrix(lib, B, N, H, Me, ld_extra, causal_off)


def test_softmax_fwd_grid_stride(lib):
    """65600 rows: every workgroup runs its row loop more than once"""
    B, N, H, Me = GRID_STRIDE
    for causal_off in (NOT_CAUSAL, 5):
        run_softmax_fwd_matrix(lib, B, N, H, Me, 0, causal_off)


# ------------------------------------------------------------------------------------------------ a. alm_xattn_softmax_bwd / dbias

def bwd_inputs(B, N, H, Me, seed):
    """P from the restatement (emask, no self part) rounded to bf16 with ZERO pad columns, as the forward kernel leaves them; dP fp32 with NaN in the columns
    >= Me (the kernels' comment: dP there was never written); ndelta random"""
    g = gen(seed)
    ldP = pad8(Me)
    emask = R.extra_mask(B, Me, g)
    P64, _, _ = R.softmax_part(uni(g, B, N, H, Me, lo=-4., hi=4.).double() / SCALE, SCALE, emask)
    P = torch.zeros((B, N, H, ldP), dtype=BF16)
    P[..., :Me] = P64.to(BF16)
    dP = torch.full((B, N, H, ldP), NAN)
    dP[..., :Me] = uni(g, B, N, H, Me, lo=-3., hi=3.)
    nd = uni(g, B, H, N, lo=-3., hi=3.)
    return P.to(dev()), dP.to(dev()), nd.to(dev()), ldP


def check_softmax_bwd(lib, B, N, H, Me):
    P, dP, nd, ldP = bwd_inputs(B, N, H, Me, 77 + Me)
    rows, lddS = B * N * H, ldP + 8
    dS = nan_buf((rows + 1, lddS), BF16)
    lib.call('alm_xattn_softmax_bwd', P.data_ptr(), ldP, dP.data_ptr(), ldP, nd.data_ptr(), SCALE, dS.data_ptr(), lddS, Me, B, N, H, lib.st())
    torch.cuda.synchronize()
    assert all_nan(dS[rows]) and all_nan(dS[:rows, ldP:]), 'dS written past ldP or past the last row'
    got = dS[:rows, :ldP].double().view(B, N, H, ldP)
    assert not bool(torch.isnan(got).any()) and float(got[..., Me:].abs().sum()) == 0., 'dS pad columns [Me, ldP) are not exactly 0'
    P64, dP64 = P[..., :Me].double(), dP[..., :Me].double()
    want = R.softmax_bwd(P64, dP64, nd.double(), SCALE)
    terms = P64 * (dP64.abs() + nd.double().abs().permute(0, 2, 1)[..., None]) * SCALE                   # the cancellation lives in dP + ndelta
    ratio = float(((got[..., :Me] - want).abs() / (EPS * terms + 1e-30)).max())
    print(f'softmax_bwd {(B, N, H, Me)}: dS err / bound {ratio:.3f}')
    assert ratio <= 1., ('dS', (B, N, H, Me), ratio)                                                  # observed on MI355X: <= 0.996 (see test_softmax_fwd)


@pytest.mark.parametrize('B,N,H,Me', SHAPES)
def test_softmax_bwd(lib, B, N, H, Me):
    check_softmax_bwd(lib, B, N, H, Me)


def test_softmax_bwd_grid_stride(lib):
    check_softmax_bwd(lib, *GRID_STRIDE)


def check_dbias(lib, B, N, H, Me):
    P, dP, nd, ldP = bwd_inputs(B, N, H, Me, 91 + Me + B)
    lddb = Me + 5
    outs = []
    for _ in range(2):
        db = nan_buf((H, N, lddb), F32)
        lib.call('alm_xattn_dbias', P.data_ptr(), ldP, dP.data_ptr(), ldP, nd.data_ptr(), db.data_ptr(), lddb, Me, B, N, H, lib.st())
        torch.cuda.synchronize()
        outs.append(db)
    assert all_nan(outs[0][..., Me:]), 'pad columns of dbias written'
    assert torch.equal(outs[0][..., :Me], outs[1][..., :Me]), 'two launches differ: the summation order is not fixed'
    P64, dP64 = P[..., :Me].double(), dP[..., :Me].double()
    want = R.dbias(P64, dP64, nd.double())
    terms = R.dbias(P64, dP64.abs(), nd.double().abs())
    ratio = float(((outs[0][..., :Me].double() - want).abs() / (terms + 1e-30)).max())
    print(f'dbias {(B, N, H, Me)}: rel. to sum of |terms| {ratio:.2e}')
    assert ratio <= 1e-4, ('dbias', (B, N, H, Me), ratio)                                             # observed on MI355X: <= 1.6e-7


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('N,H,Me', [(37, 3, 7), (50, 8, 65), (33, 5, 130)])
def test_dbias(lib, B, N, H, Me):
    check_dbias(lib, B, N, H, Me)


def test_dbias_grid_stride(lib):
    """N * H = 65600 (query, head) pairs: more than one pass of the grid"""
    check_dbias(lib, *GRID_STRIDE)


# ------------------------------------------------------------------------------------------------ a. alm_xattn_delta / combine

def check_delta(lib, B, N, H, dh):
    g = gen(5 + H + dh)
    W = H * dh
    bo, bd = torch.randn(B * N, W + 16, generator=g).to(BF16).to(dev()), torch.randn(B * N, W + 24, generator=g).to(BF16).to(dev())
    o, do = bo[:, 8:8 + W], bd[:, 16:16 + W]                                                          # ldo = W + 16, lddo = W + 24
    nd = nan_buf((B, H, N), F32)
    lib.call('alm_xattn_delta', o.data_ptr(), o.stride(0), do.data_ptr(), do.stride(0), nd.data_ptr(), B, N, H, dh, lib.st())
    torch.cuda.synchronize()
    o64, do64 = o.double().view(B, N, H, dh), do.double().view(B, N, H, dh)
    want, terms = R.delta(o64, do64), -R.delta(o64.abs(), do64.abs())
    ratio = float(((nd.double() - want).abs() / terms).max())
    print(f'delta {(B, N, H, dh)}: rel. to sum of |terms| {ratio:.2e}')
    assert ratio <= 1e-4, ('ndelta', (B, N, H, dh), ratio)                                            # observed on MI355X: <= 6.4e-8


@pytest.mark.parametrize('H', [3, 8])
@pytest.mark.parametrize('dh', [32, 64, 128])
def test_delta(lib, H, dh):
    check_delta(lib, 2, 37, H, dh)


def test_delta_grid_stride(lib):
    B, N, H, _ = GRID_STRIDE
    check_delta(lib, B, N, H, 64)


def check_combine(lib, T, H, dh, with_self):
    g = gen(11 + H + dh + with_self)
    W, ldo = H * dh, H * dh + 8
    o_e = torch.randn(T, H, dh, generator=g).to(dev())
    o_self = fself = None
    if with_self:
        buf = torch.randn(T, W + 16, generator=g).to(BF16).to(dev())
        o_self = buf[:, 8:8 + W]                                                                      # ldos = W + 16
        fself = torch.rand(T * H, generator=g).to(dev())
    out = nan_buf((T + 1, ldo), BF16)
    lib.call('alm_xattn_combine', lib.ops._p(o_self), o_self.stride(0) if with_self else 0, lib.ops._p(fself), o_e.data_ptr(), out.data_ptr(), ldo, T, H, dh, lib.st())
    torch.cuda.synchronize()
    assert all_nan(out[T]) and all_nan(out[:T, W:]), 'combine wrote a guard column or past the last token'
    e64 = o_e.double()
    s64 = None if o_self is None else o_self.double().view(T, H, dh)
    f64 = None if fself is None else fself.double().view(T, H)
    want = R.combine(s64, f64, e64)
    terms = e64.abs() if s64 is None else (f64[..., None] * s64).abs() + e64.abs()
    ratio = float(((out[:T, :W].double().view(T, H, dh) - want).abs() / (EPS * terms + 1e-30)).max())
    print(f'combine T={T} H={H} dh={dh} self={with_self}: err / bound {ratio:.3f}')
    assert ratio <= 1., ('combine', (T, H, dh, with_self), ratio)                                     # observed on MI355X: <= 0.996


@pytest.mark.parametrize('with_self', [True, False])
@pytest.mark.parametrize('H,dh', [(3, 32), (8, 32), (3, 64), (8, 64)])
def test_combine(lib, H, dh, with_self):
    check_combine(lib, 75, H, dh, with_self)


def test_combine_grid_stride(lib):
    """33000 x 8 x 16 float4 groups > 16384 workgroups x 256"""
    check_combine(lib, 33000, 8, 64, True)


# ------------------------------------------------------------------------------------------------ b. compositions

CEILING = dict(fwd=(5e-3, 3e-3), bwd=(1e-2, 4e-3))           # the flash test's own bounds (rel-max, rel-Frobenius): tests/test_gpu_kernels.py


@functools.lru_cache(maxsize=None)
def case(kind, *args, p=0.):
    """the inputs (float64, already bf16-representable), the float64 reference, the rounded model and the term magnitudes of one composition: computed once"""
    c = dict(cross=R.cross_case, prefix=R.prefix_case, dense=R.dense_case)[kind](*args)
    keep = R.keep_for(c, p) if p else None
    ref, model = R.model_and_reference(c, keep=keep, p=p)
    return c, keep, ref, model, R.term_magnitudes(c, keep=keep, p=p)


def to_rows(t):
    """(b h n d) float64 -> bf16 [B*N, H*dh] on the device"""
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * d).to(BF16).to(dev())


def from_rows(t, B, N, H):
    return t.detach().double().cpu().view(B, N, H, -1).permute(0, 2, 1, 3)


def compare(tag, name, got, ref, model, mag):
    """|got - ref| against twice |model - ref| (max and Frobenius), capped by the flash test's bound relative to the reference.  Where the reference has
    cancelled to nothing (one visible key: dS = P (dP - delta) = 0) neither is a scale: fp32 accumulation leaves ~1e-7 of the absolute terms, allowed 1e-6."""
    got = got.detach().double().cpu()
    cm, cf = CEILING['fwd' if name == 'o' else 'bwd']
    e_max, e_fro = float((got - ref).abs().max()), float((got - ref).norm())
    m_max, m_fro = float((model - ref).abs().max()), float((model - ref).norm())
    r_max, r_fro = float(ref.abs().max()), float(ref.norm())
    b_max = max(min(2 * m_max, cm * r_max), 1e-6 * float(mag.abs().max()))
    b_fro = max(min(2 * m_fro, cf * r_fro), 1e-6 * float(mag.norm()))
    if r_max <= 1e-9:                                               # no relative figures against a zero reference: print the absolute ones
        r_max = r_fro = 1.
    print(f'{tag} {name:8s} rel-max kernel {e_max / r_max:.2e} model {m_max / r_max:.2e} bound {b_max / r_max:.2e} | '
          f'rel-frob kernel {e_fro / r_fro:.2e} model {m_fro / r_fro:.2e} bound {b_fro / r_fro:.2e}')
    # model error | kernel error observed on MI355X (worst case of each test, rel-max / rel-Frobenius; the bound is 2 x model, capped):
    #   cross    o 3.69e-3 / 2.00e-3 | same     dq 4.92e-3 / 2.89e-3 | same     dke 3.06e-3 / 2.36e-3 | 3.06e-3 / 2.36e-3     dve 1.42e-3 / 1.47e-3 | same
    #            Me = 1: o exact | exact, dve exact | 3.3e-8; dq and dke are 0 | 6.0e-7 and 1.1e-6 ABSOLUTE = 1.8e-8 and 1e-9 of the terms' magnitude
    #   prefix   o 4.20e-3 / 2.55e-3 | 2.56e-3 / 2.45e-3     dq 4.66e-3 / 3.21e-3 | 5.14e-3 / 3.14e-3     dke 2.93e-3 / 3.01e-3 | 2.83e-3 / 2.94e-3
    #            dve 2.14e-3 / 1.71e-3 | same     dk_self 2.64e-3 / 2.48e-3 | 3.00e-3 / 2.39e-3     dv_self 1.85e-3 / 1.67e-3 | same
    #   dense    o 3.51e-3 / 2.43e-3     dq 6.64e-3 / 3.54e-3     dke 2.44e-3 / 2.43e-3     dve 2.25e-3 / 1.70e-3     dk_self 4.14e-3 / 3.11e-3
    #            dv_self 2.76e-3 / 1.90e-3     dbias 5.99e-3 / 2.35e-3          -- kernel | model agree to the printed digits
    #   dropout  o 4.46e-3 / 2.33e-3     dq 5.90e-3 / 3.59e-3     dke 4.76e-3 / 3.09e-3     dve 2.09e-3 / 1.79e-3     dk_self 2.65e-3 / 2.57e-3
    #            dv_self 2.05e-3 / 1.86e-3     dbias 4.33e-3 / 2.06e-3          -- kernel | model agree to the printed digits
    # (where every key runs through the xattn pieces the model's rounding points are the library's, so both land on the same bf16 numbers)
    assert e_max <= b_max and e_fro <= b_fro, (tag, name, e_max, b_max, e_fro, b_fro)


def compare_lse(tag, lse, ref):
    """the statistic is fp32 and no bf16 rounding point touches it: the single kernel's bound"""
    e = float((lse.double().cpu() - ref).abs().max())
    print(f'{tag} lse      abs {e:.2e}')
    assert e <= 1e-4, (tag, 'lse', e)                                # observed on MI355X: <= 7.3e-7


def u8(m):
    return None if m is None else m.to(U8).contiguous().to(dev())


def patch_keep(monkeypatch, lib, keep, B, N, H, M):
    """xattn._keep_mask returns the seeded draw (rows (b n h), pad columns 1: P is zero there)"""
    Mp = pad8(M)
    full = torch.ones(B * N * H, Mp)
    full[:, :M] = keep.permute(0, 2, 1, 3).reshape(B * N * H, M).float()
    calls = []

    def seeded(shape, p_, device):
        assert tuple(shape) == (B * N * H, Mp)
        calls.append(p_)
        return full.to(BF16).to(device)
    monkeypatch.setattr(lib.xattn, '_keep_mask', seeded)
    return calls


def run_xattn_only(lib, tag, c, keep, ref, model, mags, p, causal, monkeypatch=None):
    """every key through xattn.extra_attn_fwd / bwd (cross-attention and the dense math path): key set [extra | self], mask [emask | self_mask]"""
    B, H, N, dh = c['q'].shape
    ks = [t for t in (c['ke'], c['k_self']) if t is not None]
    vs = [t for t in (c['ve'], c['v_self']) if t is not None]
    k, v = torch.cat(ks, 1).to(BF16).to(dev()), torch.cat(vs, 1).to(BF16).to(dev())
    M, Me = k.shape[1], 0 if c['ke'] is None else c['ke'].shape[1]
    masks = []
    if c['ke'] is not None:
        masks.append(torch.ones(B, Me, dtype=torch.bool) if c['emask'] is None else c['emask'])
    if c['k_self'] is not None:
        masks.append(c['self_mask'])
    mask = u8(torch.cat(masks, 1))
    bias = dbias = None
    if c['bias'] is not None:
        bias = torch.full((H, N, M + 3), NAN)                        # stored wider than the key set: ldbias = shape[2] > Me, pad columns never read
        bias[..., :M] = c['bias'].float()
        bias = bias.to(dev())
        dbias = nan_buf((H, N, M), F32)
    calls = patch_keep(monkeypatch, lib, keep, B, N, H, M) if p else None
    q2, do2 = to_rows(c['q']), to_rows(c['dout'])
    o, lse, saved = lib.xattn.extra_attn_fwd(q2, k, v, mask, B, N, H, dh, c['scale'], bias=bias, causal=causal, dropout_p=p)
    nd = lib.xattn.attn_delta(o, do2, B, N, H, dh)
    dq, dk, dv = lib.xattn.extra_attn_bwd(q2, do2, saved, nd, B, N, H, dh, c['scale'], dbias=dbias)
    torch.cuda.synchronize()
    assert calls is None or calls == [p]
    compare(tag, 'o', from_rows(o, B, N, H), ref['o'], model['o'], mags['o'])
    compare_lse(tag, lse, ref['lse'])
    compare(tag, 'dq', from_rows(dq, B, N, H), ref['dq'], model['dq'], mags['dq'])
    for name, got in (('dke', dk[:, :Me]), ('dve', dv[:, :Me]), ('dk_self', dk[:, Me:]), ('dv_self', dv[:, Me:])):
        if ref[name] is not None:
            compare(tag, name, got, ref[name], model[name], mags[name])
    if dbias is not None:
        compare(tag, 'dbias', dbias, ref['dbias'], model['dbias'], mags['dbias'])                     # all columns


@pytest.mark.parametrize('B,N,H,Me,dh', R.CROSS_CASES)
def test_cross_attention_against_joint_attention(lib, B, N, H, Me, dh):
    """[null | context] keys, emask with column 0 set and (B > 1) the last batch row otherwise clear; ndelta from xattn.attn_delta.
    Model and observed kernel errors: the table in `compare`"""
    run_xattn_only(lib, f'cross{(B, N, H, Me)}', *case('cross', B, N, H, Me, dh), 0., False)


@pytest.mark.parametrize('name', R.DENSE_CASES)
def test_dense_bias_path_against_joint_attention(lib, name):
    """causal (B, H, N, dh) = (2, 4, 33, 32) with Me = N; the same behind a 5-key prefix (Me = N + 5, bias zero-padded in front); non-causal N = 64, Me = 37"""
    run_xattn_only(lib, f'dense-{name}', *case('dense', name), 0., name != 'noncausal')


# cross / non-causal cases WITHOUT the cleared batch row: with one visible key the exact dq is 0 (softmax of one score) while O = v / (1 - p) is no longer a bf16 number, so
# delta from the rounded O leaves ~2^-9 |dO| |v| in dS -- rounded_model puts dq at 6.3e-3 rel-Frobenius on (3, 33, 6, 130) with that row, above the flash
# test's ceiling for a reason that is the format's, not a kernel's.  test_cross_attention_against_joint_attention keeps the cleared row (no dropout: exact)
DROPOUT_CASES = [('cross', (3, 33, 6, 130, 64, 0, False)), ('cross', (2, 37, 8, 7, 64, 0, False)), ('dense', ('causal_prefix',)), ('dense', ('noncausal', 0, False))]


@pytest.mark.parametrize('kind,args', DROPOUT_CASES)
def test_dropout_with_the_drawn_mask_against_joint_attention(lib, kind, args, monkeypatch):
    """xattn._keep_mask pinned to a seeded draw (as tests/test_gpu_dropout.py does); the same mask goes to joint_attention.  The prefix + flash dropout
    path stays with test_gpu_dropout.py"""
    p = 0.25
    run_xattn_only(lib, f'dropout-{kind}{args}', *case(kind, *args, p=p), p, kind == 'dense' and args[0] != 'noncausal', monkeypatch)


@pytest.mark.parametrize('B,N,H,m,dh', R.PREFIX_CASES)
def test_prefix_merged_into_the_flash_result_against_joint_attention(lib, B, N, H, m, dh):
    """ops.mqa_attn_fwd, then extra_attn_fwd(o_self, lse_self); backward: ops.mqa_attn_bwd given the JOINT o and lse, then extra_attn_bwd(..., dq=dQ).
    With B > 1 the last batch row has its whole prefix masked: there o and lse are the flash kernels' own, bit for bit"""
    c, keep, ref, model, mags = case('prefix', B, N, H, m, dh)
    tag = f'prefix{(B, N, H, m)}'
    ops, xattn = lib.ops, lib.xattn
    q2, do2 = to_rows(c['q']), to_rows(c['dout'])
    kv = torch.cat((c['k_self'], c['v_self']), -1).reshape(B * N, 2 * dh).to(BF16).to(dev())            # k | v interleaved buffer: row stride 2 dh
    k, v = kv[:, :dh], kv[:, dh:]
    ke, ve = c['ke'].to(BF16).to(dev()), c['ve'].to(BF16).to(dev())
    smask, pmask = u8(c['self_mask']), u8(c['emask'])
    o_f, lse_f = ops.mqa_attn_fwd(q2, k, v, smask, B, N, H, dh)
    o, lse, saved = xattn.extra_attn_fwd(q2, ke, ve, pmask, B, N, H, dh, c['scale'], o_self=o_f, lse_self=lse_f)
    dQ, dkv = ops.mqa_attn_bwd(q2, k, v, smask, o, lse, do2, B, N, H, dh)
    nd = xattn.attn_delta(o, do2, B, N, H, dh)
    dq, dke, dve = xattn.extra_attn_bwd(q2, do2, saved, nd, B, N, H, dh, c['scale'], dq=dQ)
    torch.cuda.synchronize()
    assert dq.data_ptr() == dQ.data_ptr()
    if B > 1:
        assert not bool(c['emask'][B - 1].any())
        assert torch.equal(o[(B - 1) * N:], o_f[(B - 1) * N:]) and torch.equal(lse[B - 1], lse_f[B - 1]), 'a fully masked prefix changed the flash result'
    dkv = dkv.sum(0).view(B, N, 2 * dh)
    compare(tag, 'o', from_rows(o, B, N, H), ref['o'], model['o'], mags['o'])
    compare_lse(tag, lse, ref['lse'])
    for name, got in (('dq', from_rows(dq, B, N, H)), ('dke', dke), ('dve', dve), ('dk_self', dkv[..., :dh]), ('dv_self', dkv[..., dh:])):
        compare(tag, name, got, ref[name], model[name], mags[name])
