"""Every hyper-connection kernel of csrc/hyper.hip against the float64 restatement (tests/hc_restated.py), at every width class, stream count, storage
type and variant, with at least three rounds of the grid-stride loop, on NaN-poisoned allocations.

Case matrix (hc_restated.ROWS x factorisations x storage type): S = 4 at D 192 256 320 512 768 1000 1024, S = 2, 3 at D 256 320 512 1024; M = 6216 tokens for
D > 512 (4 waves per token, 1 token per workgroup), 12321 for D in 257..512 (2, 2), 24642 for D <= 256 (1, 4): ceil(M / TPB) >= 3 x 2048 + 1 workgroup
passes, no multiple of any grid, M % TPB != 0.  Each M as (B, N) = (3, M / 3) -- the token stride of a workgroup is below N -- and (M / 37, 37) -- the
(b, n) carry fires on most steps; plus the one-token and the (TPB + 1)-token launch.

case -> kernel instantiation (RT = storage type; `full`: D in {256, 512, 1024} fills every lane of the token's waves):
  forward  mode 2 (width, want_x and not)        hc_fwd_kernel<RT, S, WPT, false, true, false, PF>      PF = bf16 and full
           mode 2 with rin_bcast                 ... PF = false
           mode 1 (depth)                        hc_fwd_kernel<RT, S, WPT, true, false, false, PF>
           mode 3 (depth + width)                hc_fwd_kernel<RT, S, WPT, true, true, false, PF>;  with rin_bcast: PF = false
           mode 5 (final, bf16 / fp32 output)    hc_fwd_kernel<RT, S, WPT, true, false, true, PF>
  backward mode 1, stream dRn / broadcast dRn    hc_bwd_kernel<RT, S, WPT, false, true, false, ...>     bf16 and full: PF bc 0 / bc 1, else plain
           mode 2, fp32 dx                       hc_bwd_kernel<RT, S, WPT, true, false, false, ...>     bf16 and full: PF bc 0
           mode 2, fp32 dx, broadcast dRn        ...                                                   bf16 and full: PF bc 1
           mode 2, fp32 dx, broadcast R, dsum    ...  (dsum_scale = 0.375)                             bf16 and full: PF bc 2
           mode 2, fused LN, with / without extra hc_bwd_kernel<RT, S, WPT, true, false, true, ...>     bf16 and full: PF bc 0
           mode 3, fused LN, with / without extra hc_bwd_kernel<RT, S, WPT, true, true, true, ...>      bf16 and full: PF bc 0; S 4, D 1024: GL (LDS-DMA);
                                                                                                       the same with dxn / extra / y 8 bytes off: PF bc 0
           deferred finish                       hc_colsum_batched_kernel + hc_param_grads_batched_kernel<S> on the partial rows of three of the above;
                                                 full-M cases: one of the three is the (1, TPB + 1)-token launch's, so the row counts differ
  fp32 streams and the part-filled widths (192, 320, 768, 1000) always take the plain kernels (PF = false).
Every case asserts the variant it means to exercise through ops.hc_fwd_prefetch / ops.hc_bwd_variant, the launchers' own choice.

What the backward is fed: coef / mean / rstd / coef_prev come from the device forward of the same case (which test_forward holds to its bounds); the
reference backward starts from R and the parameters alone.  bf16 streams, mode 3: the kernel's width part reads the streams AS STORED (rounded to bf16),
so its reference is the float64 width connection of the device's stored R_out -- which is itself held to the float64 depth connection.

Bounds: hc_restated.TOL / TOL_SMALL (ten times the float32 CPU deviation of the restatement), in the measures described there.  The worst value seen
per kind is printed at the end of the module (information: DESIGN.md section 25 quotes it)."""
import json

import pytest
import torch

import hc_restated as H

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
WORST = {}
_T = {'tol': H.TOL, 'small': False}                 # the tolerance set of the running case (hc_restated.tolerances)


@pytest.fixture(scope='module')
def ops():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import ops as o
    yield o
    print('\nhc kernels, worst deviation per kind over bound: ' + json.dumps({k: [float('%.3g' % v), b] for k, (v, b) in sorted(WORST.items())}))


class _PoisonAlloc:
    """ops.ALLOC whose empty() hands out NaN-filled buffers: an unwritten row -- or a surplus partial row that was not cleared -- shows up as NaN
    instead of whatever the caching allocator had there before"""

    def empty(self, shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return t.fill_(float('nan')) if t.is_floating_point() else t

    def zeros(self, shape, dtype, device):
        return torch.zeros(shape, dtype=dtype, device=device)


@pytest.fixture(autouse=True)
def poisoned(ops, monkeypatch):
    monkeypatch.setattr(ops, 'ALLOC', _PoisonAlloc())


def _cases():
    out = []
    for S, D in H.ROWS:
        for B, N in H.factorisations(D) + H.small_launches(D):
            for bf in (False, True):
                out.append(pytest.param(S, D, B, N, bf, id=f'S{S}-D{D}-B{B}-N{N}-{"bf16" if bf else "fp32"}'))
    return out


_DEV, _REF = {}, {}


def _inputs(S, D, M):
    """the row's inputs on the device (fp32) and its float64 reference, kept for the cases of one (S, D, M) only"""
    key = (S, D, M)
    if key not in _DEV:
        _DEV.clear()
        _REF.clear()
        inp = H.make_inputs(S, D, M)
        _DEV[key] = H.cast_inputs(inp, F32, 'cuda')
        _REF[key] = H.all_outputs(inp, F64, 'cuda')
    return _DEV[key], _REF[key]


def _note(kind, v, bound):
    kind = kind + (' [small launch]' if _T['small'] else '')
    if v > WORST.get(kind, (-1.0, bound))[0]:
        WORST[kind] = (v, bound)


def _f32(kind, got, want, what):
    assert got.dtype == F32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    e = H.relmax(got, want)
    bound = _T['tol'][kind]
    _note(kind, e, bound)
    assert e <= bound, f'{what}: rel-max {e:.3g} > {bound:.3g}'


def _bf16(kind, got, want, what):
    assert got.dtype == BF16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    e = H.bf16_excess(got, want)
    bound = 2 * _T['tol'][kind]
    _note(kind + ' (bf16)', e, bound)
    assert e <= bound, f'{what}: beyond one bf16 rounding by {e:.3g} of max > {bound:.3g}'


def _any(kind, got, want, what):
    (_bf16 if got.dtype == BF16 else _f32)(kind, got, want, what)


def _width_outputs(r, want, S, what, want_x=True):
    rec = H.record_fields(r['coef'], S)
    for f in H.RECORD_FIELDS:
        _f32(f, rec[f], want[f], f'{what} record {f}')
    _f32('mean', r['mean'], want['mean'], what + ' mean')
    _f32('rstd', r['rstd'], want['rstd'], what + ' rstd')
    _bf16('xn', r['xn'], want['xn'], what + ' xn')
    if want_x:
        _bf16('x', r['x'], want['x'], what + ' x')
    else:
        assert r['x'] is None


def _width_ref_of_stored(R_stored_tok, hc64, g64):
    w = H.width(R_stored_tok.double(), hc64)
    return dict(w, **H.layer_norm(w['x'], g64))


def _setup(ops, S, D, B, N, bf):
    M = B * N
    i, ref = _inputs(S, D, M)
    _T.update(tol=H.tolerances(M), small=H.tolerances(M) is H.TOL_SMALL)
    rdt = BF16 if bf else F32
    t = dict(rdt=rdt, M=M,
             R0=H.to_streams(i['R0'], B, N).to(rdt), R1=H.to_streams(i['R1'], B, N).to(rdt), xb=i['xb'].contiguous(),
             hc1={k: v.contiguous() for k, v in i['hc1'].items()}, hc2={k: v.contiguous() for k, v in i['hc2'].items()},
             g1=i['g1'].contiguous(), g2=i['g2'].contiguous(), y=i['y'].to(BF16), y2=i['y2'].to(BF16),
             G=H.to_streams(i['G'], B, N).to(rdt), gb=i['gb'].contiguous(), dxn=i['dxn'].to(BF16), extra=i['extra'].to(BF16), dx=i['dx'].contiguous(),
             dbeta=i['dbeta'].contiguous())
    return i, ref, t


@pytest.mark.parametrize('S,D,B,N,bf', _cases())
def test_forward(ops, S, D, B, N, bf):
    i, ref, t = _setup(ops, S, D, B, N, bf)
    rdt, tag = t['rdt'], f'S{S} D{D} B{B} N{N} {"bf16" if bf else "fp32"}'
    toks = lambda R: H.from_streams(R, B, N)
    pf = H.expected_fwd_prefetch(D, bf)
    assert ops.hc_fwd_prefetch(D, r_dtype=rdt) == pf and not ops.hc_fwd_prefetch(D, r_dtype=rdt, rin_bcast=True)
    hc64 = {k: v.double() for k, v in t['hc2'].items()}
    # mode 2: width connection + pre-LayerNorm, with and without the bf16 copy of x
    w0 = ops.hc_fwd(t['R0'], B, S, N, D, hc=t['hc1'], ln_gamma=t['g1'], r_dtype=rdt)
    _width_outputs(w0, ref['w0'], S, tag + ' mode 2')
    _width_outputs(ops.hc_fwd(t['R0'], B, S, N, D, hc=t['hc1'], ln_gamma=t['g1'], r_dtype=rdt, want_x=False), ref['w0'], S, tag + ' mode 2 no x', want_x=False)
    # mode 1: depth connection
    d = ops.hc_fwd(t['R0'], B, S, N, D, y_prev=t['y'], coef_prev=w0['coef'], r_dtype=rdt)
    assert d['R'].dtype == rdt
    _any('R_out', toks(d['R']), ref['R_out'], tag + ' mode 1 R_out')
    # mode 3: depth + width of the next branch
    f = ops.hc_fwd(t['R0'], B, S, N, D, y_prev=t['y'], coef_prev=w0['coef'], hc=t['hc2'], ln_gamma=t['g2'], r_dtype=rdt)
    _any('R_out', toks(f['R']), ref['R_out'], tag + ' mode 3 R_out')
    _width_outputs(f, _width_ref_of_stored(toks(f['R']), hc64, t['g2'].double()) if bf else ref['wd'], S, tag + ' mode 3')
    # the first branch: one fp32 [M, D] tensor stands for every stream (never the prefetching kernel)
    wb = ops.hc_fwd(t['xb'], B, S, N, D, hc=t['hc1'], ln_gamma=t['g1'], rin_bcast=True, r_dtype=rdt)
    _width_outputs(wb, ref['wb'], S, tag + ' mode 2 rin_bcast')
    fb = ops.hc_fwd(t['xb'], B, S, N, D, y_prev=t['y'], coef_prev=wb['coef'], hc=t['hc2'], ln_gamma=t['g2'], rin_bcast=True, r_dtype=rdt)
    assert fb['R'].dtype == rdt
    _any('R_out', toks(fb['R']), ref['Rb_out'], tag + ' mode 3 rin_bcast R_out')
    _width_outputs(fb, _width_ref_of_stored(toks(fb['R']), hc64, t['g2'].double()) if bf else ref['wbd'], S, tag + ' mode 3 rin_bcast')
    # mode 5: depth + stream sum + final LayerNorm, fp32 and bf16 output
    for f32_out in (True, False):
        fin = ops.hc_fwd(t['R0'], B, S, N, D, y_prev=t['y'], coef_prev=w0['coef'], ln_gamma=t['g2'], final=True, final_f32=f32_out, r_dtype=rdt)
        what = f'{tag} mode 5 {"fp32" if f32_out else "bf16"}'
        _f32('xs', fin['xs'], ref['final']['xs'], what + ' xs')
        _f32('mean', fin['mean'], ref['final']['mean'], what + ' mean')
        _f32('rstd', fin['rstd'], ref['final']['rstd'], what + ' rstd')
        assert fin['xn'].dtype == (F32 if f32_out else BF16)
        _any('xn_final', fin['xn'], ref['final']['xn'], what + ' xn')


def _grads(got, want, what, ln):
    for k in H.GRAD_KEYS:
        if k == 'ln' and not ln:
            continue                                                       # (not a fused-LayerNorm launch: the dln slot holds zeros)
        g, w = got[k], want['grads'][k]
        assert g.dtype == F32 and g.shape == w.shape, (what, k)
        e = H.scaled_max(g, w, want['scale'][k]) if k in H.ABS_SUM_KEYS else H.relmax(g, w)
        bound = _T['tol'][k]
        _note(k, e, bound)
        assert e <= bound, f'{what} grad {k}: {e:.3g} > {bound:.3g}'


def _off8(t):
    """the same rows as a view that starts 8 bytes into a wider buffer: no longer on 16-byte boundaries"""
    wide = torch.zeros((t.shape[0], t.shape[1] + 8), dtype=t.dtype, device=t.device)
    wide[:, 4:4 + t.shape[1]] = t
    v = wide[:, 4:4 + t.shape[1]]
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize('S,D,B,N,bf', _cases())
def test_backward(ops, S, D, B, N, bf):
    i, ref, t = _setup(ops, S, D, B, N, bf)
    rdt, M, tag = t['rdt'], t['M'], f'S{S} D{D} B{B} N{N} {"bf16" if bf else "fp32"}'
    toks = lambda R: H.from_streams(R, B, N)
    tp = H.tpb(D)
    if M > 100:
        # every workgroup of the backward grid turns its loop at least three times (the forward grids are at most MAX_RESIDENT: see hc_restated.tokens)
        for mode, lnf in ((2, 0), (2, 1), (3, 1)):
            rows = ops._lib.query('alm_hc_partial_rows', mode, lnf, int(bf), S, M, D)
            niter = -(-M // tp)
            assert rows >= tp and 3 * (rows // tp) <= niter and niter % (rows // tp) != 0, (mode, lnf, rows)
    # what the forward saved: records of both branches, LayerNorm statistics (device forward of the same case, held to its bounds by test_forward)
    w0 = ops.hc_fwd(t['R0'], B, S, N, D, hc=t['hc1'], ln_gamma=t['g1'], r_dtype=rdt, want_x=False)
    w1 = ops.hc_fwd(t['R1'], B, S, N, D, hc=t['hc2'], ln_gamma=t['g2'], r_dtype=rdt, want_x=False)
    wx = ops.hc_fwd(t['xb'], B, S, N, D, hc=t['hc1'], ln_gamma=t['g1'], rin_bcast=True, r_dtype=rdt, want_x=False)
    dep = dict(y_prev=t['y'], coef_prev=w0['coef'])
    wid = dict(R=t['R1'], coef=w1['coef'], dbeta=t['dbeta'], hc=t['hc2'])
    lnk = dict(dxn=t['dxn'], mean=w1['mean'], rstd=w1['rstd'], ln_gamma=t['g2'])

    def run(kind, dRn, want, ln=False, **kw):
        what = f'{tag} {kind}'
        variant = H.expected_bwd_variant(kind.split('/')[0], S, D, bf, aligned16='off8' not in kind)
        assert ops.hc_bwd_variant(dRn, B, S, N, D, r_dtype=rdt, **kw) == variant, (what, variant)
        r = ops.hc_bwd(dRn, B, S, N, D, r_dtype=rdt, **kw)
        if want['dsum'] is not None:
            assert r['dR'] is None
            _f32('dsum', r['dsum'], want['dsum'], what + ' dsum')
        elif kw.get('hc') is not None:
            assert r['dR'].dtype == rdt
            _any('dR', toks(r['dR']), want['dR'], what + ' dR')
        if kw.get('y_prev') is not None:
            _bf16('dy', r['dy'], want['dy'], what + ' dy')
            _f32('dbeta_out', r['dbeta'], want['dbeta_out'], what + ' dbeta_out')
        if kw.get('hc') is not None and not kw.get('defer_grads'):
            _grads(r['grads'], want, what, ln)
        return r

    run('depth', t['G'], ref['b_depth'], **dep)
    run('depth_bcast', t['gb'], ref['b_depth_bcast'], bcast=True, **dep)
    run('width_dx', t['G'], dict(ref['b_dx'], dy=None), dx=t['dx'], **wid)
    run('bcast', t['gb'], ref['b_bcast'], bcast=True, dx=t['dx'], **wid)
    run('rbcast_sum', t['G'], ref['b_rbcast'], dx=t['dx'], R=t['xb'], coef=wx['coef'], dbeta=t['dbeta'], hc=t['hc1'], r_bcast=True, sum_only=True,
        dsum_scale=H.DSUM_SCALE)
    for name, extra in (('b_ln', None), ('b_ln_ex', t['extra'])):
        run('width_ln/' + name, t['G'], dict(ref[name], dy=None), ln=True, extra=extra, **lnk, **wid)
        run('fused_ln/' + name, t['G'], ref[name], ln=True, extra=extra, **lnk, **wid, **dep)
        if bf and S == 4 and D == 1024:
            # the LDS-DMA kernel above; operands that start 8 bytes off a 16-byte boundary hand over to the register-prefetch kernel
            lno = dict(lnk, dxn=_off8(t['dxn']))
            run('fused_ln/off8/' + name, t['G'], ref[name], ln=True, extra=None if extra is None else _off8(extra), **lno, **wid, y_prev=_off8(t['y']),
                coef_prev=w0['coef'])
    # the deferred finish: the partial rows of three branches (different kernels, different parameters) finished by the two batched launches.  In a launch
    # of the full token count every backward grid sits at its cap, so its three parts have the same row count; the middle part is therefore replaced by
    # the width backward of the (1, TPB + 1) launch of the same (S, D) -- 2 * TPB rows against TPB * grid -- held to ITS float64 reference
    parts = [run('fused_ln/deferred', t['G'], ref['b_ln_ex'], extra=t['extra'], defer_grads=True, **lnk, **wid, **dep),
             run('width_dx/deferred', t['G'], dict(ref['b_dx'], dy=None), dx=t['dx'], defer_grads=True, **wid),
             run('rbcast_sum/deferred', t['G'], ref['b_rbcast'], dx=t['dx'], R=t['xb'], coef=wx['coef'], dbeta=t['dbeta'], hc=t['hc1'], r_bcast=True,
                 sum_only=True, dsum_scale=H.DSUM_SCALE, defer_grads=True)]
    wants = [(ref['b_ln_ex'], True, _T['tol']), (ref['b_dx'], False, _T['tol']), (ref['b_rbcast'], False, _T['tol'])]
    if M > 100:
        parts[1], want_small = _small_deferred_part(ops, S, D, bf)
        wants[1] = (want_small, False, H.TOL_SMALL)
        assert len({p['part'][1] for p in parts}) >= 2, [p['part'][1] for p in parts]           # unequal row counts in one batched finish
    assert all(p['grads'] is None and p['part'] is not None for p in parts)
    got = ops.hc_param_grads_batched([p['part'] for p in parts], S, D)
    big = dict(_T)
    for z, (g, (want, ln, tol)) in enumerate(zip(got, wants)):
        _T.update(tol=tol, small=tol is H.TOL_SMALL)
        _grads(g, want, f'{tag} batched finish, part {z}', ln)
    _T.update(big)


def _small_deferred_part(ops, S, D, bf):
    """the deferred width backward (mode 2, fp32 dx) of the (1, TPB + 1)-token launch of a row, with its float64 reference"""
    B, N = H.small_launches(D)[1]
    inp = H.make_inputs(S, D, B * N)
    i = H.cast_inputs(inp, F32, 'cuda')
    want = H.all_outputs(inp, F64, 'cuda')['b_dx']
    rdt = BF16 if bf else F32
    hc2 = {k: v.contiguous() for k, v in i['hc2'].items()}
    R1 = H.to_streams(i['R1'], B, N).to(rdt)
    w1 = ops.hc_fwd(R1, B, S, N, D, hc=hc2, ln_gamma=i['g2'].contiguous(), r_dtype=rdt, want_x=False)
    r = ops.hc_bwd(H.to_streams(i['G'], B, N).to(rdt), B, S, N, D, dx=i['dx'].contiguous(), R=R1, coef=w1['coef'], dbeta=i['dbeta'].contiguous(), hc=hc2,
                   r_dtype=rdt, defer_grads=True)
    e = H.bf16_excess(H.from_streams(r['dR'], B, N), want['dR']) if bf else H.relmax(H.from_streams(r['dR'], B, N), want['dR'])
    assert e <= (2 if bf else 1) * H.TOL_SMALL['dR'], e
    return r, want
