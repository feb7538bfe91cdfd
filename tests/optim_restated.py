"""Float64 restatement of the fused optimiser step (csrc/optim.hip: sumsq_kernel, adam_kernel, adam_pack_kernel), written from
torch.optim.Adam / AdamW and torch.nn.utils.clip_grad_norm_ as documented -- plain numpy, no import from the package.  Also the fp32 model of
the same update (every operation rounded to fp32, no fma), which only serves to validate the per-element bounds on the CPU, and the input
generators that tests/test_optim_host.py (CPU: the model stays under the bounds) and tests/test_gpu_optim_kernels.py / test_gpu_optimizer.py
(GPU: the kernels stay under them) share, so both look at exactly the same numbers.

Bounds (per element, against adam_step; u = 2^-24, the relative half-ulp of fp32; derivation in DESIGN.md, "Fused optimiser: per-kernel tests"):
    m   4 u Mabs                          Mabs = b1 |m| + (1 - b1) (|g clip| + [L2] wd |p|)
    v   6 u V                             V    = the new second moment (every term positive)
    p   u (|p'| + |p_new|) + 12 u U       p'   = p after the decoupled decay, U = (lr / bc1) Mabs / denom
    per-chunk sum of squares  32 u relative
"""
import numpy as np

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
CHUNK = 16384                                                   # alm_opt_chunk_elems(); the GPU tests assert it
BOUND_M, BOUND_V, BOUND_P_ROUND, BOUND_P_U, BOUND_SUMSQ = 4.0, 6.0, 1.0, 12.0, 32.0
# lr and the weight decays of most shared inputs are powers of two, so the decoupled-decay factor 1 - lr wd is exact in fp32: the p bound counts the roundings
# of p' and p_new only, and the rounding of that factor (up to u / 2 relative, one more term u |p| / 2) is outside it -- with lr = 1e-3, wd = 1e-2 the fp32
# model reaches 1.09 of the bound against the float64 factor on elements whose update is far below an ulp of p.  The `prod-*` and
# `identity-prod-*` sets run the hyper-parameters training uses (PROD, WD_PROD: lr wd and 1 - lr wd both inexact in fp32, so a contraction of
# `1.f - lr * wd` that differs between code paths changes bits); their reference takes the factor as a hyper-parameter rounded to fp32 (reference_and_ratios)
HYPER = dict(lr=2.0 ** -10, beta1=0.9, beta2=0.99, eps=1e-8)
WD, WD_BIG = 2.0 ** -7, 2.0 ** -4
PROD = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8)
WD_PROD = 1e-2
# at lr = 1e-3, wd = 1e-2 the contracted and the uncontracted factor are the same fp32 number (lr wd is far below an ulp of 1: true of nearly every
# realistic pair), so those sets cannot see a contraction either; at lr = 0.1, wd = 0.3 the two differ by one ulp (fp32_decay_factors): the `split` sets
SPLIT = dict(lr=0.1, beta1=0.9, beta2=0.99, eps=1e-8)
WD_SPLIT = 0.3
# exactly representable in fp32: the rounding of the hyper-parameters to fp32 is the identity (the comparison with torch in float64)
EXACT = dict(lr=2.0 ** -10, beta1=0.875, beta2=0.984375, eps=2.0 ** -27, wd=2.0 ** -7)


def f32r(x):
    """a Python float as the C ABI receives it"""
    return float(F32(x))


def clip_coef(sumsq, max_norm, dtype=F64):
    if sumsq is None:
        return dtype(1.0)
    if dtype is F64:
        return F64(min(1.0, f32r(max_norm) / (np.sqrt(F64(sumsq)) + f32r(1e-6))))      # (sumsq: an input, the value the device scalar holds)
    return min(F32(1.0), F32(max_norm) / (np.sqrt(F32(sumsq)) + F32(1e-6)))


def adam_step(p, g, m, v, *, lr, beta1, beta2, eps, step, wd=0., decoupled=False, sumsq=None, max_norm=0., decay_factor=None):
    """one update of the fp32 arrays p, g, m, v in float64 -> dict(p, m, v, p_decayed, Mabs, U, V)"""
    p, g, m, v = (np.asarray(x, F32).astype(F64) for x in (p, g, m, v))
    return adam_step_f64(p, g, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step, wd=wd, decoupled=decoupled, sumsq=sumsq, max_norm=max_norm,
                         decay_factor=decay_factor)


def fp32_decay_factors(lr, wd):
    """the two fp32 values a kernel can hold for the decoupled-decay factor 1 - lr wd: fl(1 - fl(lr wd)) and the single-rounded fl(1 - lr wd) of a
    fused multiply-add (the compiler may contract the expression) -> list of one or two float64 values"""
    lr32, wd32 = F32(lr), F32(wd)
    two = F64(F32(1.0) - lr32 * wd32)
    one = F64(F32(1.0 - F64(lr32) * F64(wd32)))                 # (the product of two fp32 is exact in float64, 1 - x is rounded once more: to fp32 it is
    return [two] if one == two else [two, one]                  #  the fma's value except in a double-rounding tie, which the callers' hyper-parameters are not)


def adam_step_f64(p, g, m, v, *, lr, beta1, beta2, eps, step, wd=0., decoupled=False, sumsq=None, max_norm=0., decay_factor=None):
    """the formulas of adam_step on float64 arrays (the comparison with torch on float64 parameters); hyper-parameters rounded to fp32.  decay_factor:
    the decoupled-decay factor as a hyper-parameter rounded to fp32 (one of fp32_decay_factors); None: 1 - lr wd in float64"""
    lr, b1, b2, eps, wd = (F64(f32r(x)) for x in (lr, beta1, beta2, eps, wd))
    clip = clip_coef(sumsq, max_norm)
    g = g * clip
    gabs = np.abs(g)
    pd = p
    if wd != 0:
        if decoupled:
            pd = p * (1.0 - lr * wd if decay_factor is None else F64(decay_factor))
        else:
            g = g + wd * p
            gabs = gabs + wd * np.abs(p)
    m_new = b1 * m + (1.0 - b1) * g
    v_new = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** F64(step), 1.0 - b2 ** F64(step)
    denom = np.sqrt(v_new) / np.sqrt(bc2) + eps
    p_new = pd - (lr / bc1) * (m_new / denom)
    Mabs = b1 * np.abs(m) + (1.0 - b1) * gabs
    return dict(p=p_new, m=m_new, v=v_new, p_decayed=pd, Mabs=Mabs, U=(lr / bc1) * Mabs / denom, V=v_new)


def adam_step_fp32_model(p, g, m, v, *, lr, beta1, beta2, eps, step, wd=0., decoupled=False, sumsq=None, max_norm=0.):
    """the same update with every operation rounded to fp32 and no fused multiply-add except the L2 line (below; the bias corrections in double,
    rounded once, as the launcher does) -> dict(p, m, v): validates the bounds on the CPU, nothing else"""
    lr32, b1, b2, eps32, wd32 = (F32(x) for x in (lr, beta1, beta2, eps, wd))
    p, g, m, v = (np.asarray(x, F32).copy() for x in (p, g, m, v))
    one = F32(1.0)
    bc1, bc2 = 1.0 - F64(b1) ** F64(step), 1.0 - F64(b2) ** F64(step)
    step_size, inv = F32(F64(lr32) / bc1), F32(1.0 / np.sqrt(bc2))
    g = g * clip_coef(sumsq, max_norm, F32)
    if wd32 != 0:
        if decoupled:
            p = p * (one - lr32 * wd32)
        else:
            # the ONE fused operation of the model: the kernel spells this line fmaf(wd, p, g) itself (no compiler contraction involved), and the v bound
            # rests on it -- g' = g + wd p can cancel, and only a single rounding keeps its error relative to g' (hence to V = ... g'^2) instead of to
            # |g| + wd |p|.  (The product of two fp32 is exact in float64.)
            g = (g.astype(F64) + F64(wd32) * p.astype(F64)).astype(F32)
    m = b1 * m + (one - b1) * g
    v = b2 * v + ((one - b2) * g) * g
    denom = np.sqrt(v) * inv + eps32
    p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F32
    return dict(p=p, m=m, v=v)


def ratios(got, ref):
    """worst per-element error of (p, m, v) in units of each bound's terms -> dict(m, v, p): <= 1 means inside the bound"""
    tiny = 1e-300
    em = np.abs(got['m'].astype(F64) - ref['m']) / (BOUND_M * U24 * ref['Mabs'] + tiny)
    ev = np.abs(got['v'].astype(F64) - ref['v']) / (BOUND_V * U24 * ref['V'] + tiny)
    bp = BOUND_P_ROUND * U24 * (np.abs(ref['p_decayed']) + np.abs(ref['p'])) + BOUND_P_U * U24 * ref['U']
    ep = np.abs(got['p'].astype(F64) - ref['p']) / (bp + tiny)
    mx = lambda a: float(a.max()) if a.size else 0.
    return dict(m=mx(em), v=mx(ev), p=mx(ep))


def reference_and_ratios(got, t, kw, factor=None):
    """-> (adam_step's reference, ratios(got, reference)).  factor == 'fp32' (the sets at production hyper-parameters, whose 1 - lr wd is not exact in
    fp32): p' = p c with c a hyper-parameter rounded to fp32 -- whichever of the two fp32 candidates (fp32_decay_factors) fits the whole tensor; the
    bound counts the roundings of p' and p_new, not that of c, and is kept as it stands"""
    flat = [np.asarray(t[k], F32).ravel() for k in 'pgmv']
    cands = [None]
    if factor == 'fp32' and kw['decoupled'] and F32(kw['wd']) != 0:
        cands = fp32_decay_factors(kw['lr'], kw['wd'])
    best = None
    for c in cands:
        ref = adam_step(*flat, decay_factor=c, **kw)
        r = ratios(got, ref)
        if best is None or r['p'] < best[1]['p']:
            best = (ref, r)
    return best


def u_coefficient(got, ref):
    """the error of p beyond the unavoidable roundings of p' and p_new, in units of u U (the bound allows 12)"""
    ex = np.abs(got['p'].astype(F64) - ref['p']) - U24 * (np.abs(ref['p_decayed']) + np.abs(ref['p']))
    r = ex / (U24 * ref['U'] + 1e-300)
    return float(r.max()) if r.size else 0.


def exact_zero_rows(t, wd, decoupled):
    """elements with g = m = v = 0, whose update must be exact: m = v = 0, p = the decayed p (none under L2 decay, which reaches m through wd p)"""
    z = (t['g'] == 0) & (t['m'] == 0) & (t['v'] == 0)
    return z if (decoupled or F32(wd) == 0) else np.zeros_like(z)


def decayed_fp32(p, lr, wd, decoupled):
    """what an element with g = m = v = 0 must become, exactly: fl(p c) with c one of the fp32 decay factors (fl(1 - fl(lr wd)), or the single-rounded
    value where the compiler contracts 1 - lr wd into a fused multiply-add) -> list of one or two candidate arrays"""
    p = np.asarray(p, F32)
    if not decoupled or F32(wd) == 0:
        return [p.copy()]
    return [p * F32(c) for c in fp32_decay_factors(lr, wd)]


def zero_rows_exact(got_p, got_m, got_v, t, kw):
    """the exact-result rule on the elements with g = m = v = 0: m = v = 0 and p equal, bit for bit, to ONE of decayed_fp32's candidates on the whole tensor"""
    flat = {k: np.asarray(t[k]).ravel() for k in 'pgmv'}
    z = exact_zero_rows(flat, kw['wd'], kw['decoupled'])
    if not z.any():
        return True
    if got_m[z].any() or got_v[z].any():
        return False
    return any(np.array_equal(got_p[z], c[z]) for c in decayed_fp32(flat['p'], kw['lr'], kw['wd'], kw['decoupled']))


def chunk_sumsq(g, chunk=CHUNK):
    g = np.asarray(g, F32).astype(F64)
    return np.array([np.sum(g[i:i + chunk] ** 2) for i in range(0, g.size, chunk)], F64)


def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    assert not np.isnan(x).any()
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def pack_images(p_new_fp32, rows_pad, cols_pad):
    """the packed bf16 images of an UPDATED fp32 weight [rows, cols] (the kernel's own result: the images are a function of it, not of the reference)
    -> (dst [rows_pad, cols_pad], dstT [cols_pad, rows_pad]) as uint16 bit patterns, zero padded"""
    rows, cols = p_new_fp32.shape
    dst = np.zeros((rows_pad, cols_pad), np.uint16)
    dst[:rows, :cols] = bf16_bits(p_new_fp32)
    return dst, np.ascontiguousarray(dst.T)


# ------------------------------------------------------------------------------------------------------------------ shared inputs

SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, 16383, 16384, 16385, 32775, 49152)      # around the float4 tail, the 1024-element stride and CHUNK
TABLE_LENGTHS = (1, 63, 64, 65, 128, 130)                                          # around OPT_BATCH = 64
MODES = dict(adam=dict(wd=0., decoupled=False), adamw=dict(wd=WD, decoupled=True), l2=dict(wd=WD, decoupled=False))
STEPS = (1, 2, 1000, 100000)
PACK_SHAPES = ((1, 2, 2, 2, 2), (63, 126, 126, 64, 126), (64, 128, 128, 64, 128), (65, 130, 136, 66, 130), (130, 258, 258, 130, 258),
               (5, 129, 130, 6, 130), (64, 127, 128, 64, 128), (60, 100, 100, 128, 256))    # (rows, cols, ld, rows_pad, cols_pad)
PACK_JOB_COUNTS = (1, 12, 13, 25)                                                  # around PACK_BATCH = 12


def state(n, seed, gscale=1.0, zeros=True):
    """a random non-trivial optimiser state of n elements: p ~ N(0, 1), g ~ gscale N(0, 1), m ~ 0.3 gscale N(0, 1), v ~ gscale^2 U(0, 1); with `zeros`
    every 7th gradient is exactly 0 and every 11th element has g = m = v = 0 (a parameter no gradient ever reached)"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(F32)
    g = (gscale * rng.standard_normal(n)).astype(F32)
    m = (0.3 * gscale * rng.standard_normal(n)).astype(F32)
    v = (gscale * gscale * rng.random(n)).astype(F32)
    if zeros:
        g[3::7] = 0
        g[5::11] = 0
        m[5::11] = 0
        v[5::11] = 0
    return dict(p=p, g=g, m=m, v=v)


def sizes_case(seed=1, gscale=1.0):
    return [state(n, seed * 1000 + i, gscale) for i, n in enumerate(SIZES)]


def table_sizes(ntensors, empty_batch=False):
    """mostly tiny tensors; multi-chunk ones at 0, 63, 64, 127, 128 (each batch then starts at a non-zero chunk); n = 0 inside a batch; with
    `empty_batch` tensors 64..127 are all empty (a batch that launches nothing between two that do)"""
    big = {0: 16385, 63: 32775, 64: 16385, 127: 16384 + 5, 128: 32775}
    out = []
    for i in range(ntensors):
        if empty_batch and 64 <= i < 128:
            out.append(0)
        elif i in big:
            out.append(big[i])
        elif i % 9 == 4:
            out.append(0)
        else:
            out.append(1 + (i * 7) % 40)
    return out


def table_case(ntensors, empty_batch=False, seed=2):
    sizes = table_sizes(ntensors, empty_batch)
    ts = [state(n, seed * 100000 + ntensors * 200 + i) for i, n in enumerate(sizes)]
    for i, t in enumerate(ts):
        t['wd'] = (0., WD, WD_BIG)[i % 3]
        t['step'] = (0, 1, 2, 1000, 100000)[i % 5]              # 0: the launch's step
    return ts


def align_case(seed=3):
    """sizes on both sides of the float4 tail (the GPU test offsets one of p, g, m, v by 1, 2 or 3 elements)"""
    return [state(n, seed * 1000 + i) for i, n in enumerate((3, 4, 5, 1023, 1025, 16387))]


def sumsq_of(tensors):
    """fp32 sum of squares of every gradient, as the device hands it to the update"""
    return float(F32(sum(float(np.sum(t['g'].astype(F64) ** 2)) for t in tensors)))


def clip_settings(tensors):
    """name -> (sumsq, max_norm): no clipping, a norm that clips (to half), one that does not, and sumsq == 0"""
    s = sumsq_of(tensors)
    return dict(none=(None, 0.), clips=(s, 0.5 * float(np.sqrt(s))), noclip=(s, 4.0 * float(np.sqrt(s))), zero=(0., 0.5))


def pack_case(shape, seed):
    rows, cols, ld, rows_pad, cols_pad = shape
    t = state(rows * cols, seed)
    return {k: a.reshape(rows, cols) for k, a in t.items()}


def pack_mix(njobs, seed=5):
    """njobs jobs cycling through PACK_SHAPES with per-job wd and step -> list of (shape, arrays, wd, step)"""
    out = []
    for j in range(njobs):
        shape = PACK_SHAPES[(j * 3 + njobs) % len(PACK_SHAPES)]
        out.append((shape, pack_case(shape, seed * 1000 + njobs * 50 + j), (0., WD, WD_BIG)[j % 3], (0, 1, 2, 1000, 100000)[j % 5]))
    return out


def identity_case(seed=6):
    return state(4096, seed)


def make_set(tensors, *, launch_step, decoupled, sumsq=None, max_norm=0., wds=None, steps=None, shapes=None, hyper=None, factor=None):
    """one launch: `tensors` with the hyper-parameters of the launch, per-tensor weight decays and per-tensor step counts (0: the launch's);
    kws[i] are adam_step's keyword arguments for tensor i; factor: see reference_and_ratios"""
    n = len(tensors)
    hyper = dict(hyper or HYPER)
    wds = list(wds) if wds is not None else [t.get('wd', 0.) for t in tensors]
    steps = list(steps) if steps is not None else [t.get('step', 0) for t in tensors]
    kws = [dict(hyper, step=steps[i] or launch_step, wd=wds[i], decoupled=decoupled, sumsq=sumsq, max_norm=max_norm) for i in range(n)]
    return dict(tensors=tensors, kws=kws, launch_step=launch_step, decoupled=decoupled, sumsq=sumsq, max_norm=max_norm, wds=wds, steps=steps, shapes=shapes,
                hyper=hyper, factor=factor)


def _memo(fn):
    box = []

    def get(*a):
        if not box:
            box.append({})
        if a not in box[0]:
            box[0][a] = fn(*a)
        return box[0][a]
    return get


_sizes = _memo(sizes_case)
_table = _memo(table_case)
ROW_SLICES = (5, 6, 8)                                          # I, Ip, D of the two-jobs-one-parameter case (core._pack_w1)


def row_slices_case():
    I, _, D = ROW_SLICES
    return {k: a.reshape(2 * I, D) for k, a in state(2 * I * D, 77).items()}


def refused_case():
    """the 65 small tensors of the all-or-nothing test (the update is never applied to them; listed for completeness)"""
    return [state(8 + i % 5, 900 + i) for i in range(65)]


# the FusedAdam tests of tests/test_gpu_optimizer.py: name -> sizes, seeds, per-step gradient scales, optimiser arguments, max_norm
FUSED = {
    'x130': dict(sizes=tuple(table_sizes(130)), pseed=5000, gseed=6000, gstride=200, gscales=(0.01, 3.0, 0.01), lr=HYPER['lr'], wd=WD, decoupled=True, max_norm=0.5),
    'l2': dict(sizes=(1, 5, 1025, 16385, 33), pseed=5100, gseed=6100, gstride=10, gscales=(1., 1., 1.), lr=1e-3, wd=1e-2, decoupled=False, max_norm=None),
    'views': dict(sizes=(3, 4, 5, 1023, 1025, 16387), pseed=5200, gseed=6300, gstride=10, gscales=(1., 1.), lr=HYPER['lr'], wd=WD, decoupled=True, max_norm=0.5),
    'prod': dict(sizes=(5, 1025, 16385, 33), pseed=5500, gseed=6500, gstride=10, gscales=(1., 1.), lr=1e-3, wd=1e-2, decoupled=True, max_norm=0.5),
}


def fused_params(name):
    c = FUSED[name]
    return [state(n, c['pseed'] + i)['p'] for i, n in enumerate(c['sizes'])]


def fused_grads(name, it):
    c = FUSED[name]
    return [state(n, c['gseed'] + c['gstride'] * it + i, gscale=c['gscales'][it])['g'] for i, n in enumerate(c['sizes'])]


def fused_first_step(name):
    """the first step of a FusedAdam test as a launch: generated p and g, m = v = 0, step 1; the clip's sum of squares is the fp32 rounding of the
    float64 sum (the device's own differs from it by its summation error, within the 1e-5 the tests assert on the norm)"""
    c = FUSED[name]
    ts = [dict(p=p, g=g, m=np.zeros_like(p), v=np.zeros_like(p)) for p, g in zip(fused_params(name), fused_grads(name, 0))]
    s = None if c['max_norm'] is None else sumsq_of(ts)
    return make_set(ts, launch_step=1, decoupled=c['decoupled'], sumsq=s, max_norm=c['max_norm'] or 0., wds=[c['wd']] * len(ts),
                    hyper=dict(HYPER, lr=c['lr']), factor='fp32')


def _thunks():
    out = {}
    nb = len(SIZES)

    def sizes_set(mode, cname):
        base, mk = _sizes(), MODES[mode]
        s, mn = clip_settings(base)[cname]
        return make_set(base, launch_step=2, decoupled=mk['decoupled'], sumsq=s, max_norm=mn, wds=[mk['wd']] * nb)

    def step_set(st, own):
        base = _sizes()
        s, mn = clip_settings(base)['clips']
        return make_set(base, launch_step=7 if own else st, decoupled=True, sumsq=s, max_norm=mn, wds=[WD] * nb, steps=[st] * nb if own else None)

    def prod_set(cname, hyper=PROD, wd=WD_PROD):
        base = _sizes(8)
        s, mn = clip_settings(base)[cname]
        return make_set(base, launch_step=2, decoupled=True, sumsq=s, max_norm=mn, wds=[wd] * nb, hyper=hyper, factor='fp32')

    def packmix_set(nj):
        mix = pack_mix(nj)
        s = sumsq_of([a for _, a, _, _ in mix])
        return make_set([a for _, a, _, _ in mix], launch_step=3, decoupled=nj != 13, sumsq=s, max_norm=0.5 * float(np.sqrt(s)),
                        wds=[w for _, _, w, _ in mix], steps=[st for _, _, _, st in mix], shapes=[sh for sh, _, _, _ in mix])

    def identity_set(mode, cname, prod):
        t = identity_case()
        s, mn = clip_settings([t])[cname]
        mk = MODES[mode]
        if prod:
            hyper, wd = (PROD, WD_PROD) if prod == 'prod' else (SPLIT, WD_SPLIT)
            return make_set([t], launch_step=2, decoupled=True, sumsq=s, max_norm=mn, wds=[wd], hyper=hyper, factor='fp32')
        return make_set([t], launch_step=2, decoupled=mk['decoupled'], sumsq=s, max_norm=mn, wds=[mk['wd']])

    for mode in MODES:
        for cname in ('none', 'clips', 'noclip', 'zero'):
            out[f'sizes-{mode}-{cname}'] = lambda mode=mode, cname=cname: sizes_set(mode, cname)
    for st in STEPS:
        out[f'sizes-step{st}'] = lambda st=st: step_set(st, False)
        out[f'sizes-own-step{st}'] = lambda st=st: step_set(st, True)
    for gs in (1e-6, 1e3):
        for mode, mk in MODES.items():
            out[f'gscale{gs:g}-{mode}'] = lambda gs=gs, mk=mk: make_set(_sizes(4, gs), launch_step=3, decoupled=mk['decoupled'], wds=[mk['wd']] * nb)
    for cname in ('none', 'clips'):
        out[f'prod-adamw-{cname}'] = lambda cname=cname: prod_set(cname)
        out[f'split-adamw-{cname}'] = lambda cname=cname: prod_set(cname, SPLIT, WD_SPLIT)
    for nt in TABLE_LENGTHS:
        for dec in (True, False):
            out[f'table-{nt}-{"adamw" if dec else "l2"}'] = lambda nt=nt, dec=dec: make_set(_table(nt), launch_step=3, decoupled=dec)
    out['table-130-empty-batch'] = lambda: make_set(_table(130, True), launch_step=3, decoupled=True)
    out['align'] = lambda: make_set(align_case(), launch_step=2, decoupled=True, wds=[WD] * 6)
    for shape in PACK_SHAPES:
        out[f'pack-{"x".join(map(str, shape))}'] = lambda shape=shape: make_set([pack_case(shape, 7)], launch_step=2, decoupled=True, wds=[WD], shapes=[shape])
    for nj in PACK_JOB_COUNTS:
        out[f'packmix-{nj}'] = lambda nj=nj: packmix_set(nj)
    out['row-slices'] = lambda: make_set([row_slices_case()], launch_step=2, decoupled=True, wds=[WD])
    out['refused-65'] = lambda: make_set(refused_case(), launch_step=2, decoupled=True, wds=[WD] * 65)
    for mode in MODES:
        for cname in ('none', 'clips'):
            out[f'identity-{mode}-{cname}'] = lambda mode=mode, cname=cname: identity_set(mode, cname, False)
    for cname in ('none', 'clips'):
        out[f'identity-prod-adamw-{cname}'] = lambda cname=cname: identity_set('adamw', cname, 'prod')
        out[f'identity-split-adamw-{cname}'] = lambda cname=cname: identity_set('adamw', cname, 'split')
    for name in FUSED:
        out[f'fused-{name}-first-step'] = lambda name=name: fused_first_step(name)
    return out


_THUNKS = _thunks()
_BUILT = {}


def set_names(prefixes=None):
    """the names of every input set (no array is generated for this)"""
    return [n for n in _THUNKS if prefixes is None or n.startswith(prefixes)]


def input_set(name):
    """name -> make_set(...): a launch of tests/test_gpu_optim_kernels.py (or the first step of a FusedAdam test); tests/test_optim_host.py puts the fp32
    model through every one of them"""
    if name not in _BUILT:
        _BUILT[name] = _THUNKS[name]()
    return _BUILT[name]
