"""The row kernels of csrc/norm_act.hip (ln_fwd / ln_bwd at every template width, geglu_ln_fwd / geglu_ln_bwd with their two-rows-in-flight pipelines,
geglu_fwd / geglu_bwd, colsum / colsum_finish) and the loss tail of csrc/embed_ce.hip (ce_fwd, ce_bwd, reduce_sum) through direct C-ABI calls on a real
MI355X, each against the float64 restatement tests/rowops_restated.py.  The cases, inputs and tolerances are that module's: the constants are ten times
the float32 CPU model's deviation (tests/test_rowops_host.py), none comes from a GPU run.  Every leading dimension is wider than its row; every buffer a
kernel writes lies inside a sentinel-filled buffer and the sentinel -- the gaps between strided rows included -- must be intact afterwards; every case
runs twice and must be bitwise equal (no kernel here uses atomics).

Prints one line per case with the worst error / tolerance per quantity (profiles/rowops_kernels.log is such a run); a ratio above 1 fails."""
import math

import pytest
import torch

import rowops_restated as R

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD = 8                                                  # sentinel elements before and after (keeps the base 16-byte aligned for both types)
SENT = {F32: 12345.678, BF16: 1.3e36}


def _libs():
    from audiolm_pytorch_amd import _lib, ops
    return _lib, ops


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class Mat:
    """[rows, ld] of `dtype` inside ONE sentinel-filled device buffer; only the column spans are live, everything else -- the gaps between the rows and the
    guards around the matrix -- must keep the sentinel.  fill: {span index: [rows, span width] values}; unfilled live elements start as the sentinel too, so an
    element the kernel fails to write shows up as an absurd value."""

    def __init__(self, rows, ld, dtype, spans, fill=None):
        self.rows, self.ld, self.spans = rows, ld, spans
        self.host = torch.full((2 * GUARD + rows * ld,), SENT[dtype], dtype=dtype)
        self.live = torch.zeros(self.host.shape, dtype=torch.bool)
        body, lbody = self._body(self.host), self._body(self.live)
        for k, (a, b) in enumerate(spans):
            assert 0 <= a <= b <= ld
            lbody[:, a:b] = True
            if fill is not None and k in fill:
                body[:, a:b] = fill[k].to(dtype)
        self.dev = self.host.cuda()
        self.ptr = self.dev.data_ptr() + GUARD * self.host.element_size()
        assert self.ptr % 16 == 0

    def _body(self, flat):
        return flat[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)

    def view(self):
        """the device matrix as a strided torch view [rows, ld]"""
        return self._body(self.dev)

    def read(self):
        """-> the spans as the device holds them now (CPU tensors); the sentinel around them must be intact"""
        h = self.dev.cpu()
        assert torch.equal(_bits(h)[~self.live], _bits(self.host)[~self.live]), 'a kernel wrote outside its rows'
        return [self._body(h)[:, a:b].clone() for a, b in self.spans]


def mat(t, ld, dtype=None):
    """an input / output matrix with one live span of t's width"""
    return Mat(t.shape[0], ld, dtype or t.dtype, [(0, t.shape[1])], {0: t})


def out(rows, width, ld, dtype):
    return Mat(rows, ld, dtype, [(0, width)])


def vec(n):
    return Mat(1, max(n, 1), F32, [(0, n)])


def twice(run):
    """run() -> {name: CPU tensor}; two runs on fresh output buffers must agree bit for bit"""
    a, b = run(), run()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]) if a[k].dtype in (F32, BF16) else a[k], _bits(b[k]) if b[k].dtype in (F32, BF16) else b[k]), \
            f'{k}: two runs differ'
    return a


def report(name, case, ratios):
    """one log line; ratios {quantity: (measured, tolerance)}"""
    rel = {k: (v / t if t > 0 else (0.0 if v == 0 else math.inf)) for k, (v, t) in ratios.items()}
    print(f'{name:14s} {str(case):44s} ' + '  '.join(f'{k} {r:6.3f}' for k, r in rel.items()))
    bad = {k: r for k, r in rel.items() if not r <= 1.0}
    assert not bad, (name, case, bad)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd_case(case):
    _lib, _ = _libs()
    rows, D, xb, yf, xc = case
    i = R.ln_inputs(rows, D, xb)
    want = R.layer_norm_fwd(i['x'].double(), i['gamma'].double())
    gamma = i['gamma'].cuda()
    x = mat(i['x'], D + 4, BF16 if xb else F32)

    def run():
        y, c, mean, rstd = out(rows, D, D + 8, F32 if yf else BF16), (out(rows, D, D + 12, BF16) if xc else None), vec(rows), vec(rows)
        _lib.call('alm_layernorm_fwd', x.ptr, xb, D + 4, gamma.data_ptr(), y.ptr, yf, D + 8, c.ptr if xc else None, D + 12, mean.ptr, rstd.ptr, rows, D, _st())
        r = dict(y=y.read()[0], mean=mean.read()[0][0], rstd=rstd.read()[0][0])
        if xc:
            r['xcopy'] = c.read()[0]
        return r
    got = twice(run)
    x.read()                                                # the input is untouched
    if xc:
        assert torch.equal(_bits(got['xcopy']), _bits(i['x'].to(BF16))), ('xcopy is not bf16(x)', case)
    if rows >= 3:                                           # the constant row: every partial sum of 1.5 is exact
        assert bool((got['y'][1] == 0).all()) and abs(float(got['rstd'][1]) - R.LN_EPS ** -0.5) <= 1e-4 * R.LN_EPS ** -0.5, case
    report('ln_fwd', case, dict(y=(R.ratio(got['y'], want['y'], want['y_scale'], bf16=not yf), R.TOL['ln_y']),
                                mean=(R.ratio(got['mean'], want['mean'], want['mean_scale']), R.TOL['ln_mean']),
                                rstd=(R.ratio(got['rstd'], want['rstd'], want['rstd']), R.TOL['ln_rstd'])))


@pytest.mark.parametrize('D', R.LN_DS)
def test_layernorm_fwd(D):
    cases = [c for c in R.ln_fwd_cases() if c[1] == D]
    assert cases
    for c in cases:
        _ln_fwd_case(c)


def _ln_bwd_case(case):
    _lib, ops = _libs()
    rows, D, dyf, xb, dxb, ex, dg, own = case
    i = R.ln_inputs(rows, D, xb)
    gamma = i['gamma'].cuda()
    if own:                                                 # the kernel's own statistics: the reference is fed the same fp32 values
        _, _, mean, rstd = ops.layernorm_fwd(i['x'].to(BF16 if xb else F32).cuda(), gamma)
        mean, rstd = mean.cpu(), rstd.cpu()
    else:
        st = R.layer_norm_fwd(i['x'].double(), i['gamma'].double())
        mean, rstd = st['mean'].float(), st['rstd'].float()
    want = R.layer_norm_bwd(i['dy'].double(), i['x'].double(), mean.double(), rstd.double(), i['gamma'].double(), i['extra'].double() if ex else None)
    dmean, drstd = mean.cuda(), rstd.cuda()
    dy, x, extra = mat(i['dy'], D + 8, F32 if dyf else BF16), mat(i['x'], D + 4, BF16 if xb else F32), (mat(i['extra'], D + 4, BF16) if ex else None)
    nblk = _lib.query('alm_ln_partial_blocks', rows)
    assert nblk == min((rows + 3) // 4, 512)

    def run():
        dx, part = out(rows, D, D + 12, BF16 if dxb else F32), (out(nblk, D, D, F32) if dg else None)
        _lib.call('alm_layernorm_bwd', dy.ptr, dyf, D + 8, x.ptr, xb, D + 4, dmean.data_ptr(), drstd.data_ptr(), gamma.data_ptr(), extra.ptr if ex else None,
                  D + 4, dx.ptr, dxb, D + 12, part.ptr if dg else None, rows, D, _st())
        r = dict(dx=dx.read()[0])
        if dg:
            r['dgamma'] = ops.colsum(part.view()).cpu()
            part.read()
        return r
    got = twice(run)
    dy.read(), x.read()
    ratios = dict(dx=(R.ratio(got['dx'], want['dx'], want['dx_scale'], bf16=bool(dxb)), R.TOL['ln_dx']))
    if dg:
        ratios['dgamma'] = (R.ratio(got['dgamma'], want['dgamma'], want['dgamma_scale']), R.TOL['ln_dgamma'])
    report('ln_bwd', case, ratios)


@pytest.mark.parametrize('D', sorted(set(R.LN_DS + [68])))
def test_layernorm_bwd(D):
    cases = [c for c in R.ln_bwd_cases() if c[1] == D]
    assert cases
    for c in cases:
        _ln_bwd_case(c)


# ------------------------------------------------------------------------------------------------ fused GEGLU + inner LayerNorm
def _pads(rows, n, seed):
    """finite pad values, |v| <= 4, bf16"""
    g = torch.Generator().manual_seed(seed)
    return (2 * torch.randn(rows, n, generator=g)).clamp(-4, 4).to(BF16)


def _u_mat(i, rows, I, Ipad, layout, pads):
    goff, ldu, _, _ = R.geglu_layout(Ipad, layout)
    half = lambda t, seed: torch.cat([t.to(BF16), _pads(rows, Ipad - I, seed) if pads else torch.zeros(rows, Ipad - I, dtype=BF16)], 1)
    return Mat(rows, ldu, BF16, [(0, Ipad), (goff, goff + Ipad)], {0: half(i['ux'], 11), 1: half(i['ug'], 12)})


def _geglu_fwd_run(case, pads=False):
    _lib, _ = _libs()
    rows, I, Ipad, layout = case[:4]
    goff, ldu, ldo, _ = R.geglu_layout(Ipad, layout)
    i = R.geglu_inputs(rows, I)
    gamma = i['gamma'].cuda()
    u = _u_mat(i, rows, I, Ipad, layout, pads)

    def run():
        hn, mean, rstd = out(rows, Ipad, ldo, BF16), vec(rows), vec(rows)
        _lib.call('alm_geglu_ln_fwd', u.ptr, ldu, goff, gamma.data_ptr(), hn.ptr, ldo, mean.ptr, rstd.ptr, rows, I, Ipad, _st())
        return dict(hn=hn.read()[0], mean=mean.read()[0][0], rstd=rstd.read()[0][0])
    got = twice(run)
    u.read()
    return i, got


def _geglu_fwd_case(case):
    rows, I, Ipad = case[:3]
    i, got = _geglu_fwd_run(case)
    want = R.geglu_ln_fwd(i['ux'].double(), i['ug'].double(), i['gamma'].double())
    assert bool((_bits(got['hn'][:, I:]) == 0).all()), ('the pad columns of hn are not zero', case)
    report('geglu_ln_fwd', case, dict(hn=(R.ratio(got['hn'][:, :I], want['hn'], want['hn_scale'], bf16=True), R.TOL['gl_hn']),
                                      mean=(R.ratio(got['mean'], want['mean'], want['mean_scale']), R.TOL['gl_mean']),
                                      rstd=(R.ratio(got['rstd'], want['rstd'], want['rstd']), R.TOL['gl_rstd'])))


def _geglu_widths(direction):
    return sorted({c[1:3] for c in R.geglu_cases(direction)})


@pytest.mark.parametrize('I,Ipad', _geglu_widths('fwd'))
def test_geglu_ln_fwd(I, Ipad):
    for c in R.geglu_cases('fwd'):
        if c[1:3] == (I, Ipad):
            _geglu_fwd_case(c)


def _geglu_bwd_run(case, pads=False):
    _lib, ops = _libs()
    rows, I, Ipad, layout, own = case
    goff, ldu, _, lddh = R.geglu_layout(Ipad, layout)
    i = R.geglu_inputs(rows, I)
    gamma = i['gamma'].cuda()
    u = _u_mat(i, rows, I, Ipad, layout, pads)
    if own:                                                 # the kernel's own statistics: the reference is fed the same fp32 values
        _, mean, rstd = ops.geglu_ln_fwd(torch.cat([u.read()[0], u.read()[1]], 1).cuda(), gamma, I, Ipad)
        mean, rstd = mean.cpu(), rstd.cpu()
    else:
        st = R.geglu_ln_fwd(i['ux'].double(), i['ug'].double(), i['gamma'].double())
        mean, rstd = st['mean'].float(), st['rstd'].float()
    dmean, drstd = mean.cuda(), rstd.cuda()
    dpad = _pads(rows, Ipad - I, 13) if pads else torch.zeros(rows, Ipad - I, dtype=BF16)
    dhn = Mat(rows, lddh, BF16, [(0, Ipad)], {0: torch.cat([i['dhn'].to(BF16), dpad], 1)})
    nblk = _lib.query('alm_geglu_partial_blocks', rows)
    assert nblk == min(rows, 1024)

    def run():
        du, part = Mat(rows, ldu, BF16, [(0, Ipad), (goff, goff + Ipad)]), out(nblk, I, I, F32)
        _lib.call('alm_geglu_ln_bwd', dhn.ptr, lddh, u.ptr, ldu, goff, gamma.data_ptr(), dmean.data_ptr(), drstd.data_ptr(), du.ptr, part.ptr, rows, I, Ipad,
                  _st())
        dux, dug = du.read()
        r = dict(dux=dux, dug=dug, dgamma=ops.colsum(part.view()).cpu())
        part.read()
        return r
    got = twice(run)
    u.read(), dhn.read()
    return i, mean, rstd, got


def _geglu_bwd_case(case):
    rows, I, Ipad = case[:3]
    i, mean, rstd, got = _geglu_bwd_run(case)
    want = R.geglu_ln_bwd(i['dhn'].double(), i['ux'].double(), i['ug'].double(), i['gamma'].double(), mean.double(), rstd.double())
    assert bool((_bits(got['dux'][:, I:]) == 0).all()) and bool((_bits(got['dug'][:, I:]) == 0).all()), ('the pad columns of du are not zero', case)
    report('geglu_ln_bwd', case, dict(dux=(R.ratio(got['dux'][:, :I], want['dux'], want['du_scale'], bf16=True), R.TOL['gl_du']),
                                      dug=(R.ratio(got['dug'][:, :I], want['dug'], want['du_scale'], bf16=True), R.TOL['gl_du']),
                                      dgamma=(R.ratio(got['dgamma'], want['dgamma'], want['dgamma_scale']), R.TOL['gl_dgamma'])))


@pytest.mark.parametrize('I,Ipad', _geglu_widths('bwd'))
def test_geglu_ln_bwd(I, Ipad):
    for c in R.geglu_cases('bwd'):
        if c[1:3] == (I, Ipad):
            _geglu_bwd_case(c)


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_geglu_ln_never_counts_the_pad_columns(direction):
    """finite values in the pad columns [I, Ipad) of both halves of u and of dhn change no bit of any output"""
    for rows, I, Ipad, layout in R.geglu_pad_cases(direction):
        if direction == 'fwd':
            a, b = _geglu_fwd_run((rows, I, Ipad, layout))[1], _geglu_fwd_run((rows, I, Ipad, layout), pads=True)[1]
        else:
            a, b = _geglu_bwd_run((rows, I, Ipad, layout, 0))[3], _geglu_bwd_run((rows, I, Ipad, layout, 0), pads=True)[3]
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (direction, rows, I, Ipad, k)
        print(f'geglu_ln_{direction} pads ({rows}, {I}, {Ipad}, {layout}): every output bitwise equal to the zero-pad run')


# ------------------------------------------------------------------------------------------------ standalone GEGLU
@pytest.mark.parametrize('rows,I', R.GEGLU_PLAIN)
def test_geglu_plain(rows, I):
    _lib, _ = _libs()
    i = R.geglu_plain_inputs(rows, I)
    x, dy = i['x'].cuda(), i['dy'].cuda()
    (yw, ys), (dw, ds) = R.geglu_fwd(i['x'].double()), R.geglu_bwd(i['dy'].double(), i['x'].double())

    def run():
        y, dx = out(rows, I, I, F32), out(rows, 2 * I, 2 * I, F32)
        _lib.call('alm_geglu_fwd', x.data_ptr(), y.ptr, rows, I, _st())
        _lib.call('alm_geglu_bwd', dy.data_ptr(), x.data_ptr(), dx.ptr, rows, I, _st())
        return dict(y=y.read()[0], dx=dx.read()[0])
    got = twice(run)
    report('geglu', (rows, I), dict(y=(R.ratio(got['y'], yw, ys), R.TOL['ge_y']), dx=(R.ratio(got['dx'], dw, ds), R.TOL['ge_dx'])))


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_run(x_mat, ld, rows, cols, bf, scale, acc, prev, chunks):
    _lib, _ = _libs()

    def run():
        o = Mat(1, cols, F32, [(0, cols)], {0: prev.view(1, cols)})
        ws = out(chunks, cols, cols, F32) if chunks > 1 else None
        _lib.call('alm_colsum', x_mat.ptr, bf, ld, rows, cols, o.ptr, scale, acc, ws.ptr if ws else None, _st())
        if ws:
            ws.read()
        return dict(out=o.read()[0][0])
    return twice(run)['out']


@pytest.mark.parametrize('rows', R.COLSUM_ROWS)
def test_colsum(rows):
    _lib, _ = _libs()
    chunks = _lib.query('alm_colsum_chunks', rows)
    assert chunks == R.colsum_chunks(rows)
    for case in R.colsum_cases():
        if case[0] != rows:
            continue
        _, cols, bf, scale, acc = case
        i = R.colsum_inputs(rows, cols, bf)
        x = mat(i['x'], cols + 3, BF16 if bf else F32)
        got = _colsum_run(x, cols + 3, rows, cols, bf, scale, acc, i['prev'], chunks)
        want, s = R.colsum(i['x'].double(), scale, i['prev'].double() if acc else None)
        x.read()
        report('colsum', case, dict(out=(R.ratio(got, want, s), R.TOL['colsum'])))


def test_colsum_single_stage_and_partial():
    """ws == NULL on a tall input: the single-stage path; alm_colsum_partial alone: its [chunks][cols] image sums to the column sums"""
    _lib, _ = _libs()
    for rows, cols in ((3000, 65), (1025, 130), (129, 1)):
        i = R.colsum_inputs(rows, cols, 0)
        x = mat(i['x'], cols + 3)
        want, s = R.colsum(i['x'].double())
        got = _colsum_run(x, cols + 3, rows, cols, 0, 1.0, 0, i['prev'], 1)
        chunks = _lib.query('alm_colsum_chunks', rows)
        assert chunks == R.colsum_chunks(rows) > 1

        def run():
            ws = out(chunks, cols, cols, F32)
            _lib.call('alm_colsum_partial', x.ptr, cols + 3, rows, cols, ws.ptr, _st())
            return dict(ws=ws.read()[0])
        part = twice(run)['ws']
        x.read()
        report('colsum_1stage', (rows, cols), dict(out=(R.ratio(got, want, s), R.TOL['colsum']), partial=(R.ratio(part.double().sum(0), want, s), R.TOL['colsum'])))


# ------------------------------------------------------------------------------------------------ cross-entropy, reduce_sum
def _ce_case(case):
    _lib, _ = _libs()
    rows, C, ign, gs = case
    Cpad = (C + 7) // 8 * 8
    ld, ldd = Cpad + 8, Cpad + 16
    i = R.ce_inputs(rows, C, ign)
    labels = i['labels']
    want = R.cross_entropy_fwd(i['logits'].double(), labels, ign)
    lse32 = want['lse'].float()                             # the backward is fed the float64 lse rounded to fp32: forward and backward are pinned apart
    dwant = R.cross_entropy_bwd(i['logits'].double(), labels, lse32.double(), gs, ign)
    logits = Mat(rows, ld, F32, [(0, ld)], {0: torch.cat([i['logits'], torch.full((rows, ld - C), 1e9)], 1)})     # pad columns poisoned
    dlab, dlse, dgs = labels.cuda(), lse32.cuda(), torch.tensor([gs], dtype=F32).cuda()
    gs32 = float(torch.tensor(gs, dtype=F32))

    def run():
        loss, lse, d = vec(rows), vec(rows), out(rows, Cpad, ldd, BF16)
        _lib.call('alm_cross_entropy_fwd', logits.ptr, ld, dlab.data_ptr(), loss.ptr, lse.ptr, rows, C, ign, _st())
        _lib.call('alm_cross_entropy_bwd', logits.ptr, ld, dlab.data_ptr(), dlse.data_ptr(), dgs.data_ptr(), d.ptr, ldd, rows, C, Cpad, ign, _st())
        return dict(loss=loss.read()[0][0], lse=lse.read()[0][0], d=d.read()[0])
    got = twice(run)
    logits.read()
    ignored = R.ce_ignored(labels, C, ign)
    assert bool((got['loss'][ignored] == 0).all()) and bool((_bits(got['d'])[ignored] == 0).all()), ('an ignored row is not zero', case)
    assert bool((_bits(got['d'][:, C:]) == 0).all()), ('the pad columns of dlogits are not zero', case)
    dw = dwant * (gs32 / gs)                                # the kernel multiplies by the fp32 gscale
    tol = R.TOL['ce_dlogits']
    rowsum = (got['d'][:, :C].double().sum(-1).abs() - dw.sum(-1).abs()) / (2.0 ** -8 * dw.abs().sum(-1) + C * tol * gs32)
    report('cross_entropy', case, dict(loss=(R.ratio(got['loss'], want['loss'], want['scale']), R.TOL['ce_loss']),
                                       lse=(R.ratio(got['lse'], want['lse'], want['scale']), R.TOL['ce_lse']),
                                       dlogits=(R.ratio(got['d'][:, :C], dw, gs32, bf16=True), tol), rowsum=(float(rowsum.max().clamp(min=0)), 1.0)))


@pytest.mark.parametrize('C', sorted(set(R.CE_CS + [5])))
def test_cross_entropy(C):
    cases = [c for c in R.ce_cases() if c[1] == C]
    assert cases
    for c in cases:
        _ce_case(c)


def test_reduce_sum():
    _lib, _ = _libs()
    for n in R.REDUCE_NS:
        x = R.reduce_inputs(n)
        dx = x.cuda()
        want, s = R.reduce_sum(x.double(), 0.37)

        def run():
            o = vec(1)
            _lib.call('alm_reduce_sum', dx.data_ptr() if n else None, n, o.ptr, 0.37, _st())
            return dict(out=o.read()[0][0])
        got = twice(run)['out']
        if n == 0:
            assert float(got[0]) == 0.0
        report('reduce_sum', n, dict(out=(R.ratio(got[0], want, s) if n else 0.0, R.TOL['reduce_sum'])))
