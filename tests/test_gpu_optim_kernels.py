"""The three kernels of csrc/optim.hip (sumsq_kernel, adam_kernel, adam_pack_kernel) through direct C-ABI calls on a real MI355X, each against the
float64 restatement tests/optim_restated.py, per element.  Every case is ONE step from a random non-trivial state (m random, v >= 0 random), so errors
do not compound and the bounds are the rounding counts of adam_one (tests/test_optim_host.py shows the fp32 model under them on exactly
these inputs).  Every buffer is surrounded by a sentinel that is checked afterwards: nothing outside the live region may change.

Prints one line per case with the worst ratio per quantity (profiles/optim_kernels.log is such a run)."""
import numpy as np
import pytest
import torch

import optim_restated as R

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENT = np.float32(12345.678)
SENT16 = 0x7b7b                       # bf16 sentinel bit pattern of the packed images


def _libs():
    from audiolm_pytorch_amd import _lib, ops
    assert _lib.query('alm_opt_chunk_elems') == R.CHUNK
    return _lib, ops


class Arena:
    """the arrays of one quantity laid out in ONE device buffer filled with a sentinel: tensor i starts 16-byte aligned plus `off` elements (a view into
    a larger buffer at any element offset, as the flat all-reduce buckets of data-parallel training produce), at least 4 sentinel elements between
    neighbours"""

    def __init__(self, arrays, off=0):
        self.starts, cur = [], 4
        for a in arrays:
            self.starts.append(cur + off)
            cur = (cur + off + a.size + 4 + 3) // 4 * 4
        self.sizes = [a.size for a in arrays]
        self.host = np.full(cur + 4, SENT, np.float32)
        self.live = np.zeros(cur + 4, bool)
        for s, a in zip(self.starts, arrays):
            self.host[s:s + a.size] = a.ravel()
            self.live[s:s + a.size] = True
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.starts[i]

    def read(self):
        """-> the arrays as the device holds them now; the sentinel around them must be intact"""
        h = self.dev.cpu().numpy()
        assert np.array_equal(h[~self.live], self.host[~self.live]), 'a kernel wrote outside its tensors'
        return [h[s:s + n].copy() for s, n in zip(self.starts, self.sizes)]

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host.view(np.uint32))


def chunk_pairs(sizes):
    return [(i, c) for i, n in enumerate(sizes) for c in range((max(n, 0) + R.CHUNK - 1) // R.CHUNK)]


class Table:
    """AlmOptTensor table + device chunk table over four arenas; every other empty tensor has NULL pointers (an entry with n = 0 may)"""

    def __init__(self, case, offs=None, sizes=None, only_g=False):
        _lib, _ = _libs()
        offs = offs or {}
        ts = case['tensors']
        self.ar = {k: Arena([t[k] for t in ts], offs.get(k, 0)) for k in 'pgmv'}
        self.sizes = sizes if sizes is not None else [t['p'].size for t in ts]
        self.arr = (_lib.AlmOptTensor * len(ts))()
        for i, t in enumerate(ts):
            null = self.sizes[i] == 0 and i % 2 == 0
            ptr = {k: None if null or (only_g and k != 'g') else self.ar[k].ptr(i) for k in 'pgmv'}
            self.arr[i] = _lib.AlmOptTensor(ptr['p'], ptr['g'], ptr['m'], ptr['v'], self.sizes[i], case['wds'][i], case['steps'][i])
        pairs = chunk_pairs(self.sizes)
        self.nchunks = len(pairs)
        self.chunks = torch.tensor(pairs or [(0, 0)], dtype=torch.int32).reshape(-1, 2).cuda()
        self.case = case
        self.scalar = None if case['sumsq'] is None else torch.tensor(case['sumsq'], dtype=F32).cuda()

    def adam(self, nchunks=None):
        _lib, ops = _libs()
        c = self.case
        H = c['hyper']
        _lib.call('alm_opt_adam_step', self.arr, len(self.arr), self.chunks.data_ptr(), self.nchunks if nchunks is None else nchunks, H['lr'], H['beta1'],
                  H['beta2'], H['eps'], c['launch_step'], int(c['decoupled']), None if self.scalar is None else self.scalar.data_ptr(), c['max_norm'], ops._st())

    def sumsq(self):
        _lib, ops = _libs()
        guard = 8
        partial = torch.full((self.nchunks + 2 * guard,), float(SENT), dtype=F32, device='cuda')
        _lib.call('alm_opt_grad_sumsq', self.arr, len(self.arr), self.chunks.data_ptr(), self.nchunks, partial.data_ptr() + 4 * guard, ops._st())
        h = partial.cpu().numpy()
        assert (h[:guard] == SENT).all() and (h[guard + self.nchunks:] == SENT).all()
        return h[guard:guard + self.nchunks]


def check_update(name, case, got_p, got_m, got_v):
    """per element against the float64 restatement -> worst ratios (1 = at the bound); exact results where g = m = v = 0"""
    worst = dict(p=0., m=0., v=0.)
    for i, (t, kw) in enumerate(zip(case['tensors'], case['kws'])):
        got = dict(p=got_p[i].ravel(), m=got_m[i].ravel(), v=got_v[i].ravel())
        assert all(np.isfinite(got[q]).all() for q in 'pmv'), (name, i)
        _, r = R.reference_and_ratios(got, t, kw, case['factor'])
        for q in worst:
            worst[q] = max(worst[q], r[q])
        # g = m = v = 0: exact -- m = v = 0, p = fl(p c) bit for bit with c the contracted or the uncontracted fp32 factor (stricter than one ulp)
        assert R.zero_rows_exact(got['p'], got['m'], got['v'], t, kw), (name, i)
    print(f'{name:34s} GPU  m {worst["m"] * R.BOUND_M:5.2f}/4  v {worst["v"] * R.BOUND_V:5.2f}/6  p {worst["p"]:5.3f} of its bound')
    assert worst['m'] <= 1. and worst['v'] <= 1. and worst['p'] <= 1., (name, worst)
    return worst


def run_adam(name, offs=None):
    case = R.input_set(name)
    tb = Table(case, offs)
    tb.adam()
    got = {k: tb.ar[k].read() for k in 'pmv'}
    assert tb.ar['g'].unchanged()
    return check_update(name + ''.join(f'+{k}{o}' for k, o in (offs or {}).items()), case, got['p'], got['m'], got['v'])


PLAIN = R.set_names(('sizes-', 'gscale', 'prod-', 'split-', 'table-'))


@pytest.mark.parametrize('name', PLAIN)
def test_adam_kernel(name):
    """modes (Adam, AdamW, L2) x clip (none, clipping, not clipping, sumsq == 0); launch and per-tensor steps 1, 2, 1000, 100000; gradients at 1e-6 and
    1e3 of the parameter scale with planted exact zeros; AdamW at the hyper-parameters training uses (lr 1e-3, wd 1e-2) and at a pair whose decay factor
    differs by an ulp between its contracted and uncontracted form (lr 0.1, wd 0.3); tables of 1, 63, 64, 65, 128, 130 tensors (more than one batch of 64: chunk ranges that do
    not start at 0, empty tensors inside a batch, a batch of empty tensors only, per-tensor wd and step)"""
    run_adam(name)


@pytest.mark.parametrize('which', list('pgmv'))
@pytest.mark.parametrize('off', [1, 2, 3])
def test_adam_kernel_on_misaligned_views(which, off):
    """one of p, g, m, v starts 4, 8 or 12 bytes past a 16-byte boundary: the scalar path of the whole kernel"""
    run_adam('align', {which: off})


def test_adam_kernel_with_everything_misaligned():
    run_adam('align', dict(p=1, g=2, m=3, v=1))


SUMSQ_SETS = ['sizes-adam-none', 'gscale1e-06-adam', 'gscale1000-adam'] + [f'table-{n}-adamw' for n in R.TABLE_LENGTHS] + ['table-130-empty-batch']


def check_sumsq(name, case, off):
    tb = Table(case, dict(g=off), only_g=True)                 # p, m, v NULL: the sum of squares reads g only
    got = tb.sumsq().astype(np.float64)
    want = np.concatenate([R.chunk_sumsq(t['g'].ravel()) for t in case['tensors']] + [np.zeros(0)])
    assert got.shape == want.shape
    rel = np.abs(got - want) / np.where(want > 0, want, 1.)
    worst = float(rel.max() / (R.BOUND_SUMSQ * R.U24)) if rel.size else 0.
    print(f'{name + f"+g{off}":34s} GPU  per-chunk sum of squares {worst * R.BOUND_SUMSQ:5.2f}/32 u')
    assert worst <= 1. and (got[want == 0] == 0).all(), (name, worst)
    assert tb.ar['g'].unchanged()


@pytest.mark.parametrize('name', SUMSQ_SETS)
def test_sumsq_kernel(name):
    check_sumsq(name, R.input_set(name), 0)


@pytest.mark.parametrize('off', [1, 2, 3])
def test_sumsq_kernel_on_misaligned_gradients(off):
    check_sumsq('align', R.input_set('align'), off)


# ------------------------------------------------------------------------------------------------------------------ adam_pack_kernel

class PackJobs:
    """AlmOptPackJob table: every weight a [rows, cols] view with row stride ld inside a sentinel-filled buffer; images with ld_dst = cols_pad + 2 and
    ld_dstT = rows_pad + 2 inside sentinel-filled buffers that start 4 bytes (not 16) past an aligned address"""

    def __init__(self, case, images='both'):
        _lib, _ = _libs()
        self.case, self.images = case, images
        self.shapes = case['shapes']
        self.buf = {k: [] for k in 'pgmv'}
        self.host = {k: [] for k in 'pgmv'}
        self.dst, self.dstT = [], []
        self.arr = (_lib.AlmOptPackJob * len(self.shapes))()
        for j, (shape, t) in enumerate(zip(self.shapes, case['tensors'])):
            rows, cols, ld, rp, cp = shape
            ptr = {}
            for k in 'pgmv':
                h = np.full(4 + rows * ld + 4, SENT, np.float32)
                h[4:4 + rows * ld].reshape(rows, ld)[:, :cols] = t[k]
                self.host[k].append(h)
                self.buf[k].append(torch.from_numpy(h).cuda())
                ptr[k] = self.buf[k][-1].data_ptr() + 16
            d = torch.full((2 + (rp + 1) * (cp + 2),), SENT16, dtype=torch.int16, device='cuda') if images in ('both', 'dst') else None
            dT = torch.full((2 + (cp + 1) * (rp + 2),), SENT16, dtype=torch.int16, device='cuda') if images in ('both', 'dstT') else None
            self.dst.append(d)
            self.dstT.append(dT)
            self.arr[j] = _lib.AlmOptPackJob(ptr['p'], ptr['g'], ptr['m'], ptr['v'], rows, cols, ld, None if d is None else d.data_ptr() + 4, cp + 2, rp, cp,
                                             None if dT is None else dT.data_ptr() + 4, rp + 2, case['wds'][j], case['steps'][j])
        self.scalar = None if case['sumsq'] is None else torch.tensor(case['sumsq'], dtype=F32).cuda()

    def run(self):
        _lib, ops = _libs()
        c = self.case
        H = c['hyper']
        _lib.call('alm_opt_adam_pack_step', self.arr, len(self.arr), H['lr'], H['beta1'], H['beta2'], H['eps'], c['launch_step'], int(c['decoupled']),
                  None if self.scalar is None else self.scalar.data_ptr(), c['max_norm'], ops._st())

    def read(self, k, j):
        """-> the live [rows, cols] of quantity k of job j; the gaps at ld and the sentinel around the buffer must be intact"""
        rows, cols, ld, _, _ = self.shapes[j]
        h = self.buf[k][j].cpu().numpy()
        h0 = self.host[k][j]
        live = np.zeros(h.size, bool)
        live[4:4 + rows * ld].reshape(rows, ld)[:, :cols] = True
        assert np.array_equal(h[~live], h0[~live]), (k, j, 'a write into the gap at ld or outside the weight')
        if k == 'g':
            assert np.array_equal(h, h0)
        return h[4:4 + rows * ld].reshape(rows, ld)[:, :cols].copy()

    def image(self, j, transposed):
        """-> the [rows_pad, cols_pad] (or transposed) bit patterns of job j's image; everything outside it must still be the sentinel"""
        _, _, _, rp, cp = self.shapes[j]
        t = (self.dstT if transposed else self.dst)[j]
        r, c = (cp, rp) if transposed else (rp, cp)
        h = t.cpu().numpy().view(np.uint16)
        body = h[2:].reshape(r + 1, c + 2)
        assert (h[:2] == SENT16).all() and (body[r:] == SENT16).all() and (body[:, c:] == SENT16).all(), (j, transposed, 'a write outside the image')
        return body[:r, :c].copy()


def check_pack(name, images):
    _lib, ops = _libs()
    case = R.input_set(name)
    pj = PackJobs(case, images)
    pj.run()
    got = {k: [pj.read(k, j) for j in range(len(pj.shapes))] for k in 'pgmv'}
    check_update(f'{name}/{images}', case, got['p'], got['m'], got['v'])
    for j, shape in enumerate(pj.shapes):
        rows, cols, ld, rp, cp = shape
        want, wantT = R.pack_images(got['p'][j], rp, cp)             # a function of the kernel's OWN fp32 result
        master = torch.as_strided(pj.buf['p'][j], (rows, cols), (ld, 1), 4)
        ref = torch.full((rp, cp), -1, dtype=torch.int16, device='cuda').view(torch.bfloat16)
        refT = torch.full((cp, rp), -1, dtype=torch.int16, device='cuda').view(torch.bfloat16)
        ops.pack_weights_multi([(master, ref, refT, rp, cp)])         # the separate pack of the updated master
        assert np.array_equal(ref.view(torch.int16).cpu().numpy().view(np.uint16), want), (name, j)
        assert np.array_equal(refT.view(torch.int16).cpu().numpy().view(np.uint16), wantT), (name, j)
        if images in ('both', 'dst'):
            assert np.array_equal(pj.image(j, False), want), (name, j, 'dst != bf16(p_new), zero padded')
        if images in ('both', 'dstT'):
            assert np.array_equal(pj.image(j, True), wantT), (name, j, 'dstT != dst.T')


@pytest.mark.parametrize('images', ['both', 'dst', 'dstT'])
@pytest.mark.parametrize('shape', R.PACK_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adam_pack_kernel(shape, images):
    """(rows, cols, ld, rows_pad, cols_pad): one tile and less, exact tiles, one past a tile in both directions, ld > cols, an odd column count (the
    single-element branch), whole padding tiles; ld_dst > cols_pad and ld_dstT > rows_pad; either image absent"""
    check_pack('pack-' + 'x'.join(map(str, shape)), images)


@pytest.mark.parametrize('njobs', R.PACK_JOB_COUNTS)
def test_adam_pack_kernel_job_batches(njobs):
    """1, 12, 13 and 25 jobs of mixed shapes (batches of 12: the tile_end search across jobs, the second and third launch), per-job wd and step, clipping;
    13 jobs run L2 decay"""
    check_pack(f'packmix-{njobs}', 'both')


def test_adam_pack_kernel_row_slices_of_one_parameter():
    """the two halves of a GEGLU weight are two jobs that are row slices of ONE parameter and write different parts of the same images (core._pack_w1)"""
    _lib, ops = _libs()
    from audiolm_pytorch_amd import core
    I, Ip, D = R.ROW_SLICES
    case = R.input_set('row-slices')
    t, H = case['tensors'][0], case['hyper']
    dev = {k: torch.from_numpy(t[k]).cuda() for k in 'pgmv'}
    W = torch.full((2 * Ip, D), SENT16, dtype=torch.int16, device='cuda')
    WT = torch.full((D, 2 * Ip), SENT16, dtype=torch.int16, device='cuda')
    arr = (_lib.AlmOptPackJob * 2)()
    for j in range(2):
        o = j * I * D * 4
        arr[j] = _lib.AlmOptPackJob(dev['p'].data_ptr() + o, dev['g'].data_ptr() + o, dev['m'].data_ptr() + o, dev['v'].data_ptr() + o, I, D, D,
                                    W.data_ptr() + j * Ip * D * 2, D, Ip, D, WT.data_ptr() + j * Ip * 2, 2 * Ip, R.WD, 0)
    _lib.call('alm_opt_adam_pack_step', arr, 2, H['lr'], H['beta1'], H['beta2'], H['eps'], 2, 1, None, 0., ops._st())
    check_update('row-slices', case, [dev['p'].cpu().numpy()], [dev['m'].cpu().numpy()], [dev['v'].cpu().numpy()])
    refW, refWT = core._pack_w1(dev['p'], I, Ip)
    assert torch.equal(W, refW.view(torch.int16)) and torch.equal(WT, refWT.view(torch.int16))
    p_new = dev['p'].cpu().numpy()
    for j in range(2):
        want, wantT = R.pack_images(p_new[j * I:(j + 1) * I], Ip, D)
        assert np.array_equal(W[j * Ip:(j + 1) * Ip].cpu().numpy().view(np.uint16), want)
        assert np.array_equal(WT[:, j * Ip:(j + 1) * Ip].cpu().numpy().view(np.uint16), wantT)


# ------------------------------------------------------------------------------------------------------------------ the four code paths

@pytest.mark.parametrize('name', R.set_names('identity-'))
def test_the_four_code_paths_are_bit_identical(name):
    """the header's contract (alm_opt_adam_pack_step is bit-identical to alm_opt_adam_step): the same 4096 elements through adam_kernel's float4 loop,
    its scalar loop (misaligned), adam_pack_kernel's float2 branch (even cols) and its single-element branch (cols = 1, ld = 2).  Adam, AdamW and L2 at the
    shared power-of-two hyper-parameters; AdamW also at lr 1e-3, wd 1e-2 and at lr 0.1, wd 0.3, where a path that contracted `1.f - lr * wd` differently
    from the others would hold another fp32 factor and differ in nearly every element"""
    case = R.input_set(name)
    t = case['tensors'][0]
    out = {}
    for path, offs in (('float4', None), ('scalar', dict(p=1, g=1, m=1, v=1))):
        tb = Table(case, offs)
        tb.adam()
        out[path] = {k: tb.ar[k].read()[0] for k in 'pmv'}
    for path, shape in (('float2', (32, 128, 128, 32, 128)), ('single', (4096, 1, 2, 4096, 2))):
        c2 = dict(case, tensors=[{k: t[k].reshape(shape[0], shape[1]) for k in 'pgmv'}], shapes=[shape])
        pj = PackJobs(c2, 'both' if path == 'float2' else 'none')
        pj.run()
        out[path] = {k: pj.read(k, 0).ravel() for k in 'pmv'}
    check_update(name, case, [out['float4']['p']], [out['float4']['m']], [out['float4']['v']])
    for path in ('scalar', 'float2', 'single'):
        for k in 'pmv':
            same = out[path][k].view(np.uint32) == out['float4'][k].view(np.uint32)
            assert same.all(), (name, path, k, int((~same).sum()), 'elements differ from the float4 path')


# ------------------------------------------------------------------------------------------------------------------ all or nothing

@pytest.mark.parametrize('defect', ['negative-length', 'short-chunk-table'])
def test_a_refused_table_leaves_every_tensor_untouched(defect):
    """65 tensors, the defect behind the first batch of 64: AlmError, and tensors 0..63 bitwise unchanged (optimizer.py: "if it raises, nothing of this
    group has been applied yet")"""
    _lib, _ = _libs()
    case = R.input_set('refused-65')
    ts = case['tensors']
    sizes = [t['p'].size for t in ts]
    if defect == 'negative-length':
        sizes[64] = -1
    tb = Table(case, sizes=sizes)
    with pytest.raises(_lib.AlmError):
        tb.adam(tb.nchunks - 1 if defect == 'short-chunk-table' else None)
    torch.cuda.synchronize()
    for k in 'pgmv':
        assert tb.ar[k].unchanged(), (defect, k)
    with pytest.raises(_lib.AlmError):
        _lib.call('alm_opt_grad_sumsq', tb.arr, 65, tb.chunks.data_ptr(), tb.nchunks - (defect == 'short-chunk-table'), tb.ar['p'].dev.data_ptr(), None)
    assert tb.ar['p'].unchanged()
