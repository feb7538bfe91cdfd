"""Hyper-connection kernels (csrc/hyper.hip) restated in plain PyTorch, dtype-agnostic: run in float64 it is the reference of
tests/test_gpu_hc_kernels.py, run in float32 on the CPU it is the model whose deviation from float64 sets the tolerances (tests/test_hc_host.py).

Everything here is TOKEN-MAJOR: streams R [M, S, D], per-token rows [M, D], M = B * N tokens -- the arithmetic never looks at (b, n).  `to_streams` /
`from_streams` convert to and from the kernels' [B][S][N][D] image.

  width(R, hc)                 n_s = normalize(R_s) sqrt(D) (gamma + 1); alpha = tanh(n Wa) sa + Aa; beta = tanh(n wb) sb + Bb; mix_t = sum_s alpha[s][t] R_s
                               -> x = mix_0, Rp = mix_1.., and the fields of the per-token record (alpha | beta | a_pre | b_pre | rn = 1 / |R_s|)
  layer_norm(x, g)             xn = (x - mean) rstd g, rstd = 1 / sqrt(var + 1e-5)
  depth(R, alpha, beta, y)     R'_t = sum_s alpha[s][t+1] R_s + beta[t] y
  final(R, alpha, beta, y, g)  xs = sum_t R'_t, LayerNorm of xs
  backward(...)                autograd of ONE composite L = <mix[1:], G> + <xn, dxn> + <x, extra> + <beta, dbeta>  (or <x, dx> in place of the two LayerNorm
                               terms), then the depth connection of the previous branch on dR: dy = sum_t beta_k[t] dR_t, dbeta_k[t] = <dR_t, y_k>
"""
import functools
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LN_EPS, NORM_EPS = 1e-5, 1e-12
HC_KEYS = ('gamma', 'Wa', 'sa', 'Aa', 'wb', 'sb', 'Bb')
GRAD_KEYS = ('Wa', 'wb', 'gamma', 'Aa', 'Bb', 'sa', 'sb', 'ln')
ABS_SUM_KEYS = ('Aa', 'Bb', 'sa', 'sb')              # sums of cancelling per-token terms: their error is measured against sum |term|


# ------------------------------------------------------------------------------------------------ the case matrix

ROWS = [(4, 192), (4, 256), (4, 320), (4, 512), (4, 768), (4, 1000), (4, 1024), (2, 256), (2, 320), (2, 512), (2, 1024), (3, 256), (3, 320), (3, 512), (3, 1024)]
MAX_RESIDENT = 2048                                  # workgroups of 256 threads a 256-CU device can hold: 256 CUs x 32 waves / 4


def wpt(D):
    """waves per token"""
    return 1 if D <= 256 else (2 if D <= 512 else 4)


def tpb(D):
    """tokens a 256-thread workgroup works on at a time"""
    return 4 // wpt(D)


def tokens(D):
    """The smallest M = 3 * 37 * k whose ceil(M / TPB) reaches 3 * MAX_RESIDENT + 1 with M % TPB != 0 (TPB > 1): every workgroup of every possible grid
    then iterates at least 3 times, and ceil(M / TPB) = 6216 / 6161 / 6161 is no multiple of 256, hence of no grid = occupancy x CUs."""
    return {1: 111 * 56, 2: 111 * 111, 4: 111 * 222}[tpb(D)]


def factorisations(D):
    """(B, N) pairs of tokens(D): B = 3 with N > MAX_RESIDENT * TPB (the token stride of a workgroup stays below N: the batch index moves by carry only);
    N = 37 (the stride spans many sequences and 37 does not divide it: the (b, n) carry fires on most steps)."""
    M = tokens(D)
    return [(3, M // 3), (M // 37, 37)]


def small_launches(D):
    return [(1, 1), (1, tpb(D) + 1)]


def expected_fwd_prefetch(D, bf16, rin_bcast=False):
    return bool(bf16 and not rin_bcast and D == 256 * wpt(D))


def expected_bwd_variant(kind, S, D, bf16, aligned16=True):
    """kind: 'depth' (mode 1) | 'depth_bcast' | 'width_dx' (mode 2, fp32 dx) | 'width_ln' (mode 2, fused LN) | 'fused_ln' (mode 3, fused LN) |
    'bcast' (broadcast dRn, mode 2, dx) | 'rbcast_sum' (broadcast R, dsum only)"""
    if not (bf16 and D == 256 * wpt(D)):
        return 'plain'
    if kind in ('depth_bcast', 'bcast'):
        return 'pf1'
    if kind == 'rbcast_sum':
        return 'pf2'
    if kind == 'fused_ln' and S == 4 and D == 1024 and aligned16:
        return 'gl'
    return 'pf0'


# ------------------------------------------------------------------------------------------------ tolerances
# Each constant is 10 x the largest deviation of THIS restatement run in float32 on the CPU from its float64 run; the factor ten allows for another
# summation order.  The CPU run's own reductions change their order with the thread count, so it is measured with torch pinned to 4 threads, and
# tests/test_hc_host.py measures it again under the same pin and asserts <= constant / 10.  The measured value (three digits) stands beside each
# constant; the constant is ten times that value with its third digit rounded up.
# Measures (see the functions below): fp32 outputs max|got - want| / max|want| per tensor; ABS_SUM_KEYS per entry against the sum over tokens of |term|;
# bf16 outputs per element |got - want| <= 2^-8 |want| + 2 c max|want| with c the constant of the value before rounding.
# TOL: the largest deviation over the rows of ROWS at tokens(D).  TOL_SMALL: over the whole matrix, the one-token and (TPB + 1)-token launches included
# -- with one token the maximum a tensor is measured against (a single pre-activation, a single mean, one term of a "sum") can itself be a cancelled
# value, which costs up to two decimal digits; those launches are held to TOL_SMALL, every other one to the tighter TOL.
TOL = {
    'alpha': 1.19e-06,      # 1.18e-07
    'beta': 7.39e-07,       # 7.38e-08
    'a_pre': 1.02e-05,      # 1.01e-06
    'b_pre': 3.13e-06,      # 3.12e-07
    'rn': 2.10e-06,         # 2.09e-07
    'x': 1.72e-06,          # 1.71e-07
    'xn': 2.54e-06,         # 2.53e-07
    'mean': 1.88e-06,       # 1.87e-07
    'rstd': 1.98e-06,       # 1.97e-07
    'R_out': 1.74e-06,      # 1.73e-07
    'xs': 1.17e-06,         # 1.16e-07
    'xn_final': 2.28e-06,   # 2.27e-07
    # backward
    'dR': 2.72e-06,         # 2.71e-07
    'dsum': 1.98e-06,       # 1.97e-07
    'dy': 2.17e-06,         # 2.16e-07
    'dbeta_out': 9.42e-06,  # 9.41e-07
    'Wa': 8.58e-06,         # 8.57e-07
    'wb': 3.61e-05,         # 3.6e-06
    'gamma': 5.12e-06,      # 5.11e-07
    'ln': 2.00e-06,         # 1.99e-07
    'Aa': 1.02e-07,         # 1.01e-08   (of sum |d alpha|)
    'Bb': 3.67e-08,         # 3.66e-09   (of sum |d beta|)
    'sa': 6.92e-08,         # 6.91e-09   (of sum |d alpha tanh(a_pre)|)
    'sb': 5.91e-08,         # 5.9e-09   (of sum |d beta tanh(b_pre)|)
}
TOL_SMALL = {
    'alpha': 1.19e-06,      # 1.18e-07
    'beta': 7.39e-07,       # 7.38e-08
    'a_pre': 1.02e-05,      # 1.01e-06
    'b_pre': 1.73e-04,      # 1.72e-05
    'rn': 2.10e-06,         # 2.09e-07
    'x': 1.72e-06,          # 1.71e-07
    'xn': 2.54e-06,         # 2.53e-07
    'mean': 6.19e-05,       # 6.18e-06
    'rstd': 1.98e-06,       # 1.97e-07
    'R_out': 1.74e-06,      # 1.73e-07
    'xs': 1.17e-06,         # 1.16e-07
    'xn_final': 2.28e-06,   # 2.27e-07
    # backward
    'dR': 2.72e-06,         # 2.71e-07
    'dsum': 2.02e-06,       # 2.01e-07
    'dy': 2.58e-06,         # 2.57e-07
    'dbeta_out': 3.96e-05,  # 3.95e-06
    'Wa': 1.59e-05,         # 1.58e-06
    'wb': 3.61e-05,         # 3.6e-06
    'gamma': 1.46e-05,      # 1.45e-06
    'ln': 2.00e-06,         # 1.99e-07
    'Aa': 2.13e-04,         # 2.12e-05   (of sum |d alpha|)
    'Bb': 5.60e-07,         # 5.59e-08   (of sum |d beta|)
    'sa': 1.45e-05,         # 1.44e-06   (of sum |d alpha tanh(a_pre)|)
    'sb': 7.14e-05,         # 7.13e-06   (of sum |d beta tanh(b_pre)|)
}


def tolerances(M):
    return TOL_SMALL if M <= 8 else TOL


RECORD_FIELDS = ('alpha', 'beta', 'a_pre', 'b_pre', 'rn')


def relmax(got, want):
    """max|got - want| / max|want| (NaN in `got` -> inf: an unwritten element of a poisoned buffer)"""
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))


def bf16_excess(got, want):
    """per element: what of |got - want| is left after one round-to-nearest to 8 significant bits, over max|want| -- to be held to 2 c"""
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - want).abs() - 2.0 ** -8 * want.abs()).max().clamp(min=0.) / want.abs().max().clamp(min=1e-300))


def scaled_max(got, want, scale):
    """per entry |got - want| / scale (the absolute-sum scale of a cancelling sum)"""
    got, want, scale = got.double(), want.double(), scale.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - want).abs() / scale.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------ layout

def to_streams(R_tok, B, N):
    """[M, S, D] -> the kernels' [B, S, N, D]"""
    M, S, D = R_tok.shape
    return R_tok.view(B, N, S, D).permute(0, 2, 1, 3).contiguous()


def from_streams(R, B, N):
    """[B, S, N, D] -> [M, S, D]"""
    return R.permute(0, 2, 1, 3).reshape(B * N, R.shape[1], R.shape[3])


def record_fields(coef, S):
    """the kernel's per-token record [M, 2 S (S + 1) + 3 S] -> dict of its five fields (Coef<S> of csrc/hyper.hip)"""
    M = coef.shape[0]
    nb = S * (S + 1)
    o = [0, nb, nb + S, 2 * nb + S, 2 * nb + 2 * S, 2 * nb + 3 * S]
    assert coef.shape[1] == o[-1]
    return dict(alpha=coef[:, o[0]:o[1]].reshape(M, S, S + 1), beta=coef[:, o[1]:o[2]], a_pre=coef[:, o[2]:o[3]].reshape(M, S, S + 1),
                b_pre=coef[:, o[3]:o[4]], rn=coef[:, o[4]:o[5]])


# ------------------------------------------------------------------------------------------------ forward

def width(R, hc):
    """R [M, S, D] -> dict(x [M, D], Rp [M, S, D], alpha [M, S, S+1], beta [M, S], a_pre, b_pre, rn [M, S])"""
    M, S, D = R.shape
    rn = 1.0 / R.norm(dim=-1, keepdim=True).clamp(min=NORM_EPS)           # F.normalize's eps clamp
    normed = R * rn * math.sqrt(D) * (hc['gamma'] + 1)
    a_pre = normed @ hc['Wa']
    b_pre = normed @ hc['wb']
    alpha = torch.tanh(a_pre) * hc['sa'] + hc['Aa']
    beta = torch.tanh(b_pre) * hc['sb'] + hc['Bb']
    mix = torch.einsum('mst,msd->mtd', alpha, R)
    return dict(x=mix[:, 0], Rp=mix[:, 1:], alpha=alpha, beta=beta, a_pre=a_pre, b_pre=b_pre, rn=rn.squeeze(-1))


def layer_norm(x, g):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + LN_EPS).rsqrt()
    return dict(xn=(x - mean) * rstd * g, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1))


def depth(R, alpha, beta, y):
    return torch.einsum('mst,msd->mtd', alpha[:, :, 1:], R) + beta.unsqueeze(-1) * y.unsqueeze(1)


def final(R, alpha, beta, y, g):
    xs = depth(R, alpha, beta, y).sum(1)
    return dict(xs=xs, **layer_norm(xs, g))


# ------------------------------------------------------------------------------------------------ backward

def backward(R1, hc, G, dbeta, *, ln_gamma=None, dxn=None, extra=None, dx=None, y_k=None, beta_k=None, r_bcast=False, g_bcast=False, dsum_scale=1.0,
             width_part=True):
    """alm_hc_bwd restated.  R1 [M, S, D] (r_bcast: [M, D], every stream equals it), G [M, S, D] (g_bcast: [M, D]).  Fused LayerNorm: dxn (+ extra) and
    ln_gamma; otherwise dx.  y_k / beta_k: the depth connection of the previous branch.  width_part False: mode 1 (dR = G).
    -> dict(dR [M, S, D], dsum [M, D] (r_bcast), grads {8 keys}, scale {Aa, Bb, sa, sb}, dy, dbeta_out)"""
    out = dict(grads=None, scale=None, dsum=None, dy=None, dbeta_out=None)
    S = hc['Aa'].shape[0] if hc is not None else (beta_k.shape[1])
    Gs = G.unsqueeze(1).expand(-1, S, -1) if g_bcast else G
    if width_part:
        leaf = R1.detach().clone().requires_grad_(True)
        R = leaf.unsqueeze(1).expand(-1, S, -1) if r_bcast else leaf
        p = {k: hc[k].detach().clone().requires_grad_(True) for k in HC_KEYS}
        w = width(R, p)
        for k in ('alpha', 'beta'):
            w[k].retain_grad()
        L = (w['Rp'] * Gs).sum() + (w['beta'] * dbeta).sum()
        lng = None
        if dx is not None:
            L = L + (w['x'] * dx).sum()
        else:
            lng = ln_gamma.detach().clone().requires_grad_(True)
            L = L + (layer_norm(w['x'], lng)['xn'] * dxn).sum()
            if extra is not None:
                L = L + (w['x'] * extra).sum()
        L.backward()
        grads = {k: p[k].grad for k in HC_KEYS}
        grads['ln'] = lng.grad if lng is not None else None
        da, db = w['alpha'].grad, w['beta'].grad
        out['grads'] = grads
        out['scale'] = dict(Aa=da.abs().sum(0), Bb=db.abs().sum(0), sa=(da * torch.tanh(w['a_pre'].detach())).abs().sum(),
                            sb=(db * torch.tanh(w['b_pre'].detach())).abs().sum())
        if r_bcast:
            out['dsum'] = leaf.grad * dsum_scale
            dR = None
        else:
            dR = leaf.grad
    else:
        dR = Gs
    out['dR'] = dR
    if y_k is not None:
        out['dy'] = torch.einsum('mt,mtd->md', beta_k, dR)
        out['dbeta_out'] = torch.einsum('mtd,md->mt', dR, y_k)
    return out


# ------------------------------------------------------------------------------------------------ inputs

def _hc(S, D, gen):
    """the 7 parameters of one connection, every one carrying signal; Wa / wb width-scaled as tests/golden/common.py does (pre-activation std 0.4 at every D:
    a fixed 0.05 randn gives 1.6 at D = 1024, where tanh saturates and its gradient vanishes)"""
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F32)
    ws = 0.05 * math.sqrt(64.0 / max(64, D))
    # static_alpha: the branch-input column is 1, 1/2, 1/3 .. (every stream feeds x, their sum stays away from zero: with the broadcast input x is
    # (sum_s alpha[s][0]) xb, and a column of zero + noise lets the LayerNorm variance of some token collapse)
    col = (1.0 / (1 + torch.arange(S, dtype=F32))).view(S, 1)
    return dict(gamma=0.1 * r(D), Wa=ws * r(D, S + 1), sa=(0.1 + 0.02 * r(1)).reshape(()),
                Aa=torch.cat([col, torch.eye(S)], 1) + 0.1 * r(S, S + 1), wb=ws * r(D), sb=(0.1 + 0.02 * r(1)).reshape(()),
                Bb=1 + 0.1 * r(S))


@functools.lru_cache(maxsize=2)
def make_inputs(S, D, M, seed=0):
    """Every input of every case of one matrix row, token-major, fp32 CPU tensors (identical for both storage types: whatever a bf16 kernel reads as
    bf16 -- streams, y, dxn, extra -- is bf16-representable).  The streams differ in scale (0.6 .. 1.5) so that no two carry the same norm."""
    gen = torch.Generator().manual_seed(1000 * S + D + 7919 * seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F32)
    b = lambda t: t.to(BF16).to(F32)
    sc = (0.6 + 0.3 * torch.arange(S, dtype=F32)).view(1, S, 1)
    return dict(
        S=S, D=D, M=M,
        R0=b(r(M, S, D) * sc), R1=b(r(M, S, D) * sc + 0.25), xb=r(M, D) + 0.1,
        hc1=_hc(S, D, gen), hc2=_hc(S, D, gen), g1=1 + 0.1 * r(D), g2=1 + 0.1 * r(D),
        y=b(r(M, D)), y2=b(r(M, D)),
        G=b(r(M, S, D)), gb=r(M, D), dxn=b(r(M, D)), extra=b(0.5 * r(M, D)), dx=r(M, D), dbeta=r(M, S))


def cast_inputs(inp, dtype, device=None):
    def c(v):
        if isinstance(v, dict):
            return {k: c(x) for k, x in v.items()}
        return v.to(device=device, dtype=dtype) if isinstance(v, torch.Tensor) else v
    return c(inp)


def input_conditions(inp):
    """what the inputs must satisfy for the tolerances to mean something (float64): the pre-activation std (tanh neither linear nor saturated), the
    smallest stream norm over the mean norm, the smallest LayerNorm variance"""
    i = cast_inputs(inp, F64)
    out = {}
    for name, R, hc in (('0', i['R0'], i['hc1']), ('1', i['R1'], i['hc2']), ('b', i['xb'].unsqueeze(1).expand(-1, inp['S'], -1), i['hc1'])):
        w = width(R, hc)
        nrm = 1.0 / w['rn']
        x = w['x']
        out[name] = dict(pre_std=float(torch.cat([w['a_pre'].flatten(), w['b_pre'].flatten()]).std()), min_norm=float(nrm.min() / nrm.mean()),
                         min_var=float(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1).min()))
    return out


# ------------------------------------------------------------------------------------------------ every output of a row, in one precision

def all_outputs(inp, dtype, device=None):
    """Every case of one matrix row on one set of inputs, in `dtype`: what the GPU tests compare the kernels with (float64) and what the host test measures
    the float32 deviation of.  Forward: width of R0 (hc1) and of R1 (hc2), their LayerNorms, depth, depth + width, final, the rin_bcast form.
    Backward: fused LN with and without extra (+ depth), fp32 dx (+ depth), depth only, broadcast dRn, broadcast R + scaled stream sum."""
    i = cast_inputs(inp, dtype, device)
    o = {}
    with torch.no_grad():
        w0 = width(i['R0'], i['hc1'])
        w1 = width(i['R1'], i['hc2'])
        o['w0'] = dict(w0, **layer_norm(w0['x'], i['g1']))
        o['w1'] = dict(w1, **layer_norm(w1['x'], i['g2']))
        o['R_out'] = depth(i['R0'], w0['alpha'], w0['beta'], i['y'])                    # modes 1 and 3
        wd = width(o['R_out'], i['hc2'])
        o['wd'] = dict(wd, **layer_norm(wd['x'], i['g2']))                               # mode 3 (fp32 streams)
        o['final'] = final(i['R0'], w0['alpha'], w0['beta'], i['y'], i['g2'])            # mode 5
        Rb = i['xb'].unsqueeze(1).expand(-1, inp['S'], -1)
        wb = width(Rb, i['hc1'])                                                         # first branch: every stream equals xb
        o['wb'] = dict(wb, **layer_norm(wb['x'], i['g1']))
        o['Rb_out'] = depth(Rb, wb['alpha'], wb['beta'], i['y'])
        wbd = width(o['Rb_out'], i['hc2'])
        o['wbd'] = dict(wbd, **layer_norm(wbd['x'], i['g2']))
        beta_k = w0['beta']
    kw = dict(y_k=i['y'], beta_k=beta_k)
    o['b_ln_ex'] = backward(i['R1'], i['hc2'], i['G'], i['dbeta'], ln_gamma=i['g2'], dxn=i['dxn'], extra=i['extra'], **kw)
    o['b_ln'] = backward(i['R1'], i['hc2'], i['G'], i['dbeta'], ln_gamma=i['g2'], dxn=i['dxn'], **kw)
    o['b_dx'] = backward(i['R1'], i['hc2'], i['G'], i['dbeta'], dx=i['dx'], **kw)
    o['b_depth'] = backward(None, None, i['G'], None, width_part=False, **kw)
    o['b_depth_bcast'] = backward(None, None, i['gb'], None, width_part=False, g_bcast=True, **kw)
    o['b_bcast'] = backward(i['R1'], i['hc2'], i['gb'], i['dbeta'], dx=i['dx'], g_bcast=True)
    o['b_rbcast'] = backward(i['xb'], i['hc1'], i['G'], i['dbeta'], dx=i['dx'], r_bcast=True, dsum_scale=DSUM_SCALE)
    return o


DSUM_SCALE = 0.375


def deviations(got, want):
    """all_outputs in two precisions -> {kind of TOL: worst deviation in that kind's measure}"""
    dev = {k: 0.0 for k in TOL}

    def up(kind, v):
        dev[kind] = max(dev[kind], v)
    for name in ('w0', 'w1', 'wd', 'wb', 'wbd'):
        for f in RECORD_FIELDS + ('x', 'xn', 'mean', 'rstd'):
            up(f, relmax(got[name][f], want[name][f]))
    for name in ('R_out', 'Rb_out'):
        up('R_out', relmax(got[name], want[name]))
    up('xs', relmax(got['final']['xs'], want['final']['xs']))
    up('xn_final', relmax(got['final']['xn'], want['final']['xn']))
    up('mean', relmax(got['final']['mean'], want['final']['mean']))
    up('rstd', relmax(got['final']['rstd'], want['final']['rstd']))
    for name in ('b_ln_ex', 'b_ln', 'b_dx', 'b_depth', 'b_depth_bcast', 'b_bcast', 'b_rbcast'):
        g, w = got[name], want[name]
        if w['dsum'] is not None:
            up('dsum', relmax(g['dsum'], w['dsum']))
        elif name not in ('b_depth', 'b_depth_bcast'):
            up('dR', relmax(g['dR'], w['dR']))
        if w['dy'] is not None:
            up('dy', relmax(g['dy'], w['dy']))
            up('dbeta_out', relmax(g['dbeta_out'], w['dbeta_out']))
        if w['grads'] is not None:
            for k in GRAD_KEYS:
                if w['grads'][k] is None:
                    continue
                if k in ABS_SUM_KEYS:
                    up(k, scaled_max(g['grads'][k], w['grads'][k], w['scale'][k]))
                else:
                    up(k, relmax(g['grads'][k], w['grads'][k]))
    return dev
