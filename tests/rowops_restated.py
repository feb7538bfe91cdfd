"""The row kernels of csrc/norm_act.hip (gamma-only LayerNorm, fused GEGLU + inner LayerNorm, standalone GEGLU, column sums) and the loss tail of
csrc/embed_ce.hip (cross-entropy forward / backward, reduce_sum) restated in plain PyTorch, dtype-agnostic: run in float64 it is the reference of
tests/test_gpu_rowops_kernels.py, run in float32 on the CPU it is the model whose deviation from float64 sets the tolerances (tests/test_rowops_host.py).

The kernels' rounding points are kept: whatever a kernel reads as bf16 is bf16-representable in the inputs (it enters exactly); statistics are two-pass
(mean, then centred squares) with the divisor D / I and eps = 1e-5 inside the root; a bf16 output is the fp32 value rounded once, so every function here
returns the value BEFORE that rounding and the measures below allow one round-to-nearest on top of the fp32 tolerance.

  layer_norm_fwd(x, g)                          y = (x - mean) rstd g, mean, rstd
  layer_norm_bwd(dy, x, mean, rstd, g, extra)   dx = rstd (dy g - c1 - xhat c2) (+ extra), dgamma = sum_rows dy xhat
  geglu_ln_fwd(ux, ug, g)                       h = gelu(ug) ux, then layer_norm_fwd(h)  (fp64: exact erf; otherwise A&S 7.1.26 as common.hpp writes it)
  geglu_ln_bwd(dhn, ux, ug, g, mean, rstd)      du (x half | gate half), dgamma
  geglu_fwd / geglu_bwd                         the standalone module on fp32 rows (exact erf in every precision: the kernel calls erff)
  colsum, cross_entropy_fwd, cross_entropy_bwd, reduce_sum
"""
import functools
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LN_EPS = 1e-5
GE_MAX_PAD = 3072                                     # the widest padded inner width the fused GEGLU kernels take


# ------------------------------------------------------------------------------------------------ tolerances
# Each constant is 10 x the largest deviation of THIS restatement run in float32 on the CPU (4 torch threads) from its float64 run over the whole case
# matrix below, in the measure named beside it; the factor ten allows for another summation order and for the GPU's exp / rcp / rsqrt.  The measured
# value stands in the trailing comment; tests/test_rowops_host.py measures it again and asserts model <= constant / 10 (1 + 1e-2).  No constant comes
# from a GPU run.  bf16 outputs: per element |got - want| <= 2^-8 |want| + TOL scale (one round-to-nearest to 8 significant bits plus the fp32 term).
TOL = {
    'ln_y': 2.10e-06,        # 2.09e-07   of max|g| rstd (max|x - mean| + mean|x|), per row
    'ln_mean': 2.48e-06,     # 2.48e-07   of mean|x|, per row
    'ln_rstd': 2.69e-06,     # 2.69e-07   relative, per row
    'ln_dx': 1.55e-06,       # 1.54e-07   of the row's dx scale (layer_norm_bwd)
    'ln_dgamma': 1.64e-06,   # 1.64e-07   of sum_rows |dy xhat|, per column
    'gl_hn': 2.56e-06,       # 2.55e-07   of max|g| rstd (max|h - mean| + mean|ug ux|), per row
    'gl_mean': 1.95e-06,     # 1.95e-07   of mean|ug ux|, per row
    'gl_rstd': 2.27e-05,     # 2.27e-06   relative, per row
    'gl_du': 4.22e-06,       # 4.21e-07   of the row's du scale (geglu_ln_bwd)
    'gl_dgamma': 1.58e-06,   # 1.58e-07   of sum_rows |dhn| (|xhat| + |ug ux| rstd), per column
    'ge_y': 1.26e-06,        # 1.25e-07   of max|x gate|, per row
    'ge_dx': 1.77e-06,       # 1.77e-07   of max(max|dy gate|, max|dy x|), per row
    'colsum': 7.92e-07,      # 7.91e-08   of |prev| + |scale| sum_rows |x|, per column
    'reduce_sum': 1.70e-07,  # 1.7e-08    of |scale| sum |x|
    'ce_loss': 1.63e-06,     # 1.62e-07   of max(1, max finite |logit|), per row
    'ce_lse': 6.32e-07,      # 6.32e-08   likewise
    'ce_dlogits': 8.86e-07,  # 8.86e-08   of |gscale|
}


def ratio(got, want, scale, bf16=False):
    """max over elements of (|got - want| - [bf16] 2^-8 |want|) / scale; a non-finite element of `got` where `want` is finite -> inf.  To be held to TOL."""
    got, want = got.double(), want.double()
    scale = torch.as_tensor(scale, dtype=F64)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    if bf16:
        err = (err - 2.0 ** -8 * want.abs()).clamp(min=0.)
    return float((err / scale.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------ sums in a kernel-like order
def seq_sum0(t):
    """sum over dim 0 the way one thread of a kernel does it: one accumulator, in order, in t's precision"""
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def colsum_chunks(rows):
    """alm_colsum_chunks"""
    return 1 if rows <= 128 else min(16, (rows + 63) // 64)


def colsum_partial(x, chunks):
    """stage 1 of the column sums: [chunks, cols]; a chunk's rows go to 4 row lanes (row % 4), each summed in order, then (l0 + l1) + (l2 + l3)"""
    rows, cols = x.shape
    rpc = (rows + chunks - 1) // chunks if rows else 0
    out = []
    for k in range(chunks):
        sub = x[k * rpc:min(rows, (k + 1) * rpc)]
        pad = (-sub.shape[0]) % 4
        sub = torch.cat([sub, sub.new_zeros(pad, cols)]).view(-1, 4, cols)
        lane = seq_sum0(sub) if sub.shape[0] else sub.new_zeros(4, cols)
        out.append((lane[0] + lane[1]) + (lane[2] + lane[3]))
    return torch.stack(out)


def colsum(x, scale=1.0, prev=None, two_stage=True):
    """out[c] = (prev[c] +) scale sum_r x[r][c];  -> (out, the absolute-sum scale |prev| + |scale| sum_r |x|)"""
    part = colsum_partial(x, colsum_chunks(x.shape[0]) if two_stage else 1)
    v = seq_sum0(part) * scale
    s = x.abs().sum(0) * abs(scale)
    return (v, s) if prev is None else (prev + v, s + prev.abs())


def reduce_sum(x, scale=1.0):
    """-> (scale sum x, |scale| sum |x|): 1024 threads stride the input, then a tree"""
    n = x.numel()
    if n == 0:
        return x.new_zeros(()), x.new_zeros(())
    t = torch.cat([x, x.new_zeros((-n) % 1024)]).view(-1, 1024)
    return seq_sum0(t).sum() * scale, x.abs().sum() * abs(scale)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layer_norm_fwd(x, g, mutant=None):
    """-> dict(y, mean, rstd, y_scale [rows, 1], mean_scale [rows]).  y_scale = max|g| rstd (max|x - mean| + mean|x|): an error d of the mean moves y by
    d rstd g, and the mean's own error is a rounding of sum |x| / D -- the row's condition, without which a row of std 1e-3 around 3 would set the tolerance
    of every row."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if mutant == 'one_pass':
        var = (x * x).mean(-1, keepdim=True) - mean * mean
    else:
        var = ((x - mean) ** 2).sum(-1, keepdim=True) / ((D - 1) if mutant == 'div_dm1' else D)
    rstd = 1.0 / (var.sqrt() + LN_EPS) if mutant == 'eps_outside' else (var + LN_EPS).rsqrt()
    absmean = x.abs().mean(-1, keepdim=True)
    return dict(y=(x - mean) * rstd * g, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), y_scale=g.abs().max() * rstd * ((x - mean).abs().max(-1, keepdim=True)[0] + absmean),
                mean_scale=absmean.squeeze(-1))


def layer_norm_bwd(dy, x, mean, rstd, g, extra=None):
    """mean / rstd [rows] are inputs (the forward's, whatever precision they were rounded to).  -> dict(dx, dgamma, dx_scale [rows, 1], dgamma_scale [D]).
    c1 = mean(dy g) and c2 = mean(dy g xhat) are sums that cancel: dx is measured against rstd (max|gg| + mean|gg| + max|xhat| mean|gg xhat|) (+ max|extra|),
    dgamma against sum_rows |dy xhat| (x, mean and rstd are exact inputs, so every term carries a relative error only)."""
    mean, rstd = mean.unsqueeze(-1), rstd.unsqueeze(-1)
    xhat = (x - mean) * rstd
    gg = dy * g
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xhat).mean(-1, keepdim=True)
    dx = rstd * (gg - c1 - xhat * c2)
    amax = lambda t: t.abs().max(-1, keepdim=True)[0]
    scale = rstd.abs() * (amax(gg) + gg.abs().mean(-1, keepdim=True) + amax(xhat) * (gg * xhat).abs().mean(-1, keepdim=True))
    if extra is not None:
        dx = dx + extra
        scale = scale + amax(extra)
    dgamma = colsum(dy * xhat)[0]
    return dict(dx=dx, dgamma=dgamma, dx_scale=scale, dgamma_scale=(dy * xhat).abs().sum(0))


# ------------------------------------------------------------------------------------------------ GEGLU
def gauss_cdf_pdf(v, exact):
    """cdf = 0.5 (1 + erf(v / sqrt 2)), pdf = exp(-v^2 / 2) / sqrt(2 pi).  exact False: gauss_cdf_pdf of csrc/common.hpp, Abramowitz & Stegun 7.1.26."""
    if exact:
        return 0.5 * (1 + torch.erf(v * 0.70710678118654752)), 0.3989422804014327 * torch.exp(-0.5 * v * v)
    ax = v.abs() * 0.70710678118654752
    ex = torch.exp(-ax * ax)
    t = 1.0 / (0.3275911 * ax + 1.0)
    poly = t * (t * (t * (t * (t * 1.061405429 - 1.453152027) + 1.421413741) - 0.284496736) + 0.254829592)
    return 0.5 * (1.0 + torch.copysign(1.0 - poly * ex, v)), 0.3989422804014327 * ex


def _gelu(ug, exact, mutant=None):
    if mutant == 'tanh_gelu':
        return 0.5 * ug * (1 + torch.tanh(0.7978845608028654 * (ug + 0.044715 * ug ** 3)))
    return ug * gauss_cdf_pdf(ug, exact)[0]


def geglu_ln_fwd(ux, ug, g, exact=None, mutant=None, Ipad=None):
    """ux, ug [rows, I] (the valid columns of the two halves of u), g [I] -> dict(h, mean, rstd, hn, hn_scale, mean_scale).  exact None: exact erf in float64,
    the kernel's polynomial otherwise.  Ipad: only the mutants need it.  h = ug ux cdf with cdf in [0, 1] carrying an ABSOLUTE error (a gate of -12 gives
    h = 1e-32 |ux|, which no fp32 cdf resolves), so the scales are built on |ug ux|: mean_scale = mean|ug ux|, hn_scale = max|g| rstd (max|h - mean| + mean|ug ux|)."""
    exact = (ux.dtype == F64) if exact is None else exact
    I = ux.shape[-1]
    h = _gelu(ug, exact, mutant) * ux
    if mutant == 'drop4':                                    # the 4th component of the last 4-vector reads as zero
        c = (I - 1) // 4 * 4 + 3
        if c < I:
            h = h.clone()
            h[:, c] = 0
    div = Ipad if mutant == 'div_ipad' else I
    mean = h.sum(-1, keepdim=True) / div
    sq = ((h - mean) ** 2).sum(-1, keepdim=True)
    if mutant == 'pad_in_mean':                              # the centred squares of the pad columns (h = 0 there) counted too
        sq = sq + (Ipad - I) * mean * mean
    rstd = (sq / div + LN_EPS).rsqrt()
    absmean = (ug * ux).abs().mean(-1, keepdim=True)
    return dict(h=h, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), hn=(h - mean) * rstd * g,
                hn_scale=g.abs().max() * rstd * ((h - mean).abs().max(-1, keepdim=True)[0] + absmean),
                mean_scale=absmean.squeeze(-1))


def geglu_ln_bwd(dhn, ux, ug, g, mean, rstd, exact=None, mutant=None):
    """-> dict(dux, dug [rows, I], dgamma [I], du_scale [rows, 1], dgamma_scale [I]); mean / rstd [rows] are inputs.  du = dh * (d h / d u) with dh the
    LayerNorm backward of h: measured against the dx scale of layer_norm_bwd times max(max|ug|, max|ux|), the bound of the row's |d h / d u| up to 1.13;
    dgamma against sum_rows |dhn| (|xhat| + |ug ux| rstd): h inside xhat carries the cdf's absolute error times |ug ux|."""
    exact = (ux.dtype == F64) if exact is None else exact
    if mutant == 'stale_stats':                              # the statistics of the NEXT row (a prefetch buffer that was not swapped)
        mean, rstd = mean.roll(-1), rstd.roll(-1)
    cdf, pdf = gauss_cdf_pdf(ug, exact)
    gl = ug * cdf
    gb = ux * (ug * pdf + cdf)
    mean, rstd = mean.unsqueeze(-1), rstd.unsqueeze(-1)
    xhat = (gl * ux - mean) * rstd
    gg = dhn * g
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xhat).mean(-1, keepdim=True)
    dh = rstd * (gg - c1 - xhat * c2)
    amax = lambda t: t.abs().max(-1, keepdim=True)[0]
    sdh = rstd.abs() * (amax(gg) + gg.abs().mean(-1, keepdim=True) + amax(xhat) * (gg * xhat).abs().mean(-1, keepdim=True))
    dgamma = colsum(dhn * xhat)[0]
    return dict(dux=dh * gl, dug=dh * gb, dgamma=dgamma, du_scale=sdh * torch.maximum(amax(ug), amax(ux)),
                dgamma_scale=(dhn.abs() * (xhat.abs() + (ug * ux).abs() * rstd.abs())).sum(0))


def geglu_fwd(x):
    """the standalone module: x [rows, 2 I] fp32 (x half | gate half) -> (y [rows, I], the row scale max|x gate| [rows, 1]: the cdf's error is absolute)"""
    I = x.shape[-1] // 2
    y = x[:, :I] * _gelu(x[:, I:], True)
    return y, (x[:, :I] * x[:, I:]).abs().max(-1, keepdim=True)[0]


def geglu_bwd(dy, x):
    """-> (dx [rows, 2 I], the row scale max(max|dy gate|, max|dy x|) [rows, 1])"""
    I = x.shape[-1] // 2
    cdf, pdf = gauss_cdf_pdf(x[:, I:], True)
    dx = torch.cat([dy * x[:, I:] * cdf, dy * x[:, :I] * (cdf + x[:, I:] * pdf)], -1)
    return dx, torch.maximum((dy * x[:, I:]).abs().max(-1, keepdim=True)[0], (dy * x[:, :I]).abs().max(-1, keepdim=True)[0])


# ------------------------------------------------------------------------------------------------ cross-entropy
def ce_ignored(labels, C, ignore_index):
    return (labels == ignore_index) | (labels < 0) | (labels >= C)


def cross_entropy_fwd(logits, labels, ignore_index, mutant=None):
    """logits [rows, C] (valid columns), labels int64 [rows] -> dict(loss [rows], lse [rows], scale [rows] = max(1, the row's largest finite |logit|)).
    A label equal to ignore_index, negative or >= C is ignored: loss 0."""
    C = logits.shape[-1]
    ign = ce_ignored(labels, C, ignore_index)
    if mutant == 'no_max':
        lse = logits.exp().sum(-1).log()
    else:
        mx = logits.max(-1, keepdim=True)[0]
        lse = mx.squeeze(-1) + (logits - mx).exp().sum(-1).log()
    picked = logits.gather(1, labels.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    loss = torch.where(ign, torch.zeros_like(lse), lse - picked)
    fin = torch.where(torch.isfinite(logits), logits.abs(), torch.zeros_like(logits))
    return dict(loss=loss, lse=lse, scale=fin.max(-1)[0].clamp(min=1.0))


def cross_entropy_bwd(logits, labels, lse, gscale, ignore_index, mutant=None):
    """-> dlogits [rows, C] = (exp(logit - lse) - [c == label]) gscale, ignored rows zero.  Its scale is |gscale| (a probability is <= 1)."""
    C = logits.shape[-1]
    ign = ce_ignored(labels, C, ignore_index)
    onehot = torch.zeros_like(logits)
    valid = (labels >= 0) & (labels < C) & (~ign if mutant != 'label_on_ignored' else torch.ones_like(ign))
    onehot[valid, labels[valid]] = 1
    d = ((logits - lse.unsqueeze(-1)).exp() * (~ign).unsqueeze(-1) - onehot) * gscale
    return d


# ------------------------------------------------------------------------------------------------ the case matrix
LN_DS = [4, 8, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2044, 2048]
LN_ROWS = [1, 3, 37]
LN_FWD_COMBOS = [(xb, yf, xc) for xb in (0, 1) for yf in (0, 1) for xc in (0, 1)]            # (x bf16, y fp32, xcopy)
LN_BWD_COMBOS = [(1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]                         # (dy fp32, x bf16, dx bf16): the five the launcher takes


def ln_fwd_cases():
    """(rows, D, x_bf16, y_f32, xcopy): every D of every template class edge at 1 / 3 / 37 rows, the combinations cycling; 16389 rows (4096 blocks x 4 waves
    + 5: the grid-stride loop runs twice, the second pass ragged); all 8 type combinations at D = 260 and 1028"""
    out, k = [], 0
    for D in LN_DS:
        for rows in LN_ROWS:
            out.append((rows, D) + LN_FWD_COMBOS[k % 8])
            k += 3                                            # 3 is coprime to 8: every combination comes up at every row count
    out += [(16389, 8, 0, 0, 1), (16389, 8, 1, 1, 0), (16389, 260, 0, 0, 1), (16389, 260, 1, 1, 0)]
    out += [(37, D) + c for D in (260, 1028) for c in LN_FWD_COMBOS]
    return out


def ln_bwd_cases():
    """(rows, D, dy_f32, x_bf16, dx_bf16, extra, dgamma, own_stats): 2051 / 4100 rows are 512 blocks x 4 waves + 3 / x 2 + 4 (a wave accumulates 2 - 3 rows,
    the last pass ragged)"""
    out, k = [], 0
    for D in LN_DS:
        for rows in LN_ROWS:
            out.append((rows, D) + LN_BWD_COMBOS[k % 5] + (k % 2, (k // 2) % 2, 0))
            k += 1
    out += [(37, 260) + c + (ex, dg, 0) for c in LN_BWD_COMBOS for ex in (0, 1) for dg in (0, 1)]
    k = 0
    for rows in (2051, 4100):
        for D in (68, 1028):
            out.append((rows, D) + LN_BWD_COMBOS[k % 5] + (k % 2, 1, 0))
            k += 1
    out += [(4100, 68, 0, 1, 1, 1, 1, 0), (37, 516, 0, 0, 0, 1, 1, 1), (37, 516, 0, 1, 1, 0, 1, 1)]
    return out


GEGLU_WIDTHS = [(1, 8), (3, 8), (4, 8), (5, 8), (7, 8), (8, 8), (5, 16), (170, 176), (681, 688), (1021, 1024), (1024, 1024), (1027, 1032), (2045, 2048),
                (2048, 2048), (2051, 2056), (2730, 2736), (3065, 3072), (3072, 3072)]
GEGLU_PIPE_WIDTHS = [(5, 8), (681, 688)]
GEGLU_FWD_PIPE_ROWS = [2049, 4097, 4100, 6145]      # grid 2048: blocks doing 1-2, 2-3, 2-3 (4 blocks 3), 3-4 rows: the loop leaves after either register set
GEGLU_BWD_PIPE_ROWS = [1025, 2049, 2050, 3073]      # grid 1024: likewise
GEGLU_WIDE = (2730, 2736, 2051)
GEGLU_PAD_CASES = [(19, 5, 16, 1), (19, 681, 688, 0)]                                           # + one pipeline case per direction, see geglu_pad_cases


def geglu_layout(Ipad, layout):
    """-> (gate_offset, ldu, ldo, lddh)"""
    return (Ipad, 2 * Ipad, Ipad, Ipad) if layout == 0 else (Ipad + 8, 2 * Ipad + 24, Ipad + 8, Ipad + 16)


def geglu_cases(direction):
    """(rows, I, Ipad, layout, own_stats)"""
    out = [(rows, I, Ip, (k + j) % 2, 0) for k, (I, Ip) in enumerate(GEGLU_WIDTHS) for j, rows in enumerate((1, 19))]
    pipe = GEGLU_FWD_PIPE_ROWS if direction == 'fwd' else GEGLU_BWD_PIPE_ROWS
    out += [(rows, I, Ip, (k + j) % 2, 0) for k, (I, Ip) in enumerate(GEGLU_PIPE_WIDTHS) for j, rows in enumerate(pipe)]
    out.append((GEGLU_WIDE[2],) + GEGLU_WIDE[:2] + (1, 0))
    if direction == 'bwd':
        out += [(19, 681, 688, 1, 1), (1025, 5, 8, 0, 1)]
    return out


def geglu_pad_cases(direction):
    return GEGLU_PAD_CASES + [((2049 if direction == 'fwd' else 1025), 5, 8, 1)]


GEGLU_PLAIN = [(1, 1), (7, 5), (37, 682), (4099, 513)]                                          # 4099 * 513 > 8192 * 256: the grid-stride loop iterates

COLSUM_ROWS = [1, 4, 5, 16, 17, 128, 129, 1024, 1025, 3000]
COLSUM_COLS = [1, 63, 64, 65, 130]
COLSUM_MODES = [(1.0, 0), (0.37, 0), (-2.5, 1)]                                                  # (scale, accumulate)


def colsum_cases():
    """(rows, cols, bf16, scale, accumulate)"""
    out, k = [], 0
    for rows in COLSUM_ROWS:
        for cols in COLSUM_COLS:
            for bf in (0, 1):
                out.append((rows, cols, bf) + COLSUM_MODES[k % 3])
                k += 1
    return out


CE_CS = [1, 2, 21, 63, 64, 65, 1025]
CE_GSCALES = [0.37, 1.0 / 4096]


def ce_cases():
    """(rows, C, ignore_index, gscale); 32773 rows = 8192 blocks x 4 waves + 5"""
    out = [(rows, C, (-1, 3)[(k + j) % 2], CE_GSCALES[(k + j // 2) % 2]) for k, C in enumerate(CE_CS) for j, rows in enumerate((1, 45, 45))]
    return out + [(32773, 5, 3, 0.37), (32773, 5, -1, 1.0 / 4096)]


REDUCE_NS = [0, 1, 63, 1023, 1024, 1025, 5000, 100003]


# ------------------------------------------------------------------------------------------------ inputs (fp32 CPU tensors, seeded)
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 7919 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _b(t):
    return t.to(BF16).to(F32)


@functools.lru_cache(maxsize=4)
def ln_inputs(rows, D, x_bf16):
    """per row: mean ~ N(0, 3^2), std from {1e-3, 0.5, 4}; with >= 3 rows, row 1 is the constant 1.5 (y = 0, rstd = eps^-1/2: every partial sum of 1.5 is exact)
    and row 2 carries one outlier of 1e4.  dy / extra are bf16-representable (an fp32 dy reads the same values)."""
    gen = _gen(1, rows, D, x_bf16)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F32)
    std = torch.tensor([1e-3, 0.5, 4.0])[torch.randint(0, 3, (rows,), generator=gen)].unsqueeze(1)
    x = 3 * r(rows, 1) + std * r(rows, D)
    if rows >= 3:
        x[1] = 1.5
        x[2, D // 2] = 1e4
    if x_bf16:
        x = _b(x)
    return dict(x=x, gamma=1 + 0.2 * r(D), dy=_b(r(rows, D)), extra=_b(0.5 * r(rows, D)))


GATE_EXTREMES = [38.0, -38.0, 1e4, -1e4, 37.75, -37.75, 9984.0, -9984.0]                        # bf16 values where exp(-v^2 / 2) underflows


def gate_rows(rows, I, gen, bf16=True):
    """row % 3 == 0: randn; == 1: a sweep over [-12, 12] that starts with +0 and -0; row 2: the extremes.  One row: the sweep."""
    g = torch.randn(rows, I, generator=gen, dtype=F32)
    sweep = torch.linspace(-12, 12, I) if I > 1 else torch.tensor([-12.0])
    sweep = sweep[torch.randperm(I, generator=gen)].clone()
    if I > 2:
        sweep[0], sweep[1] = 0.0, -0.0
    if rows == 1:
        g[0] = sweep
    g[1::3] = sweep
    if rows >= 3:
        g[2] = torch.tensor(GATE_EXTREMES).repeat((I + 7) // 8)[:I]
    return _b(g) if bf16 else g


@functools.lru_cache(maxsize=2)
def geglu_inputs(rows, I):
    """the valid columns of the two halves of u, dhn (all bf16-representable), gamma"""
    gen = _gen(2, rows, I)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F32)
    return dict(ux=_b(2 * r(rows, I) + 0.5), ug=gate_rows(rows, I, gen), dhn=_b(r(rows, I)), gamma=1 + 0.2 * r(I))


def geglu_plain_inputs(rows, I):
    gen = _gen(3, rows, I)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F32)
    return dict(x=torch.cat([2 * r(rows, I) + 0.5, gate_rows(rows, I, gen, bf16=False)], 1), dy=r(rows, I))


def colsum_inputs(rows, cols, bf16):
    """columns of mixed sign and scale whose sum nearly cancels (the last row is minus the sum of the others, rounded)"""
    gen = _gen(4, rows, cols, bf16)
    x = torch.randn(rows, cols, generator=gen, dtype=F32) * (10.0 ** (4 * torch.rand(rows, 1, generator=gen) - 2))
    if rows > 1:
        x[-1] = -x[:-1].double().sum(0).float()
    return dict(x=_b(x) if bf16 else x, prev=torch.randn(cols, generator=gen, dtype=F32))


def reduce_inputs(n):
    gen = _gen(5, n)
    x = torch.randn(n, generator=gen, dtype=F32) * (10.0 ** (4 * torch.rand(n, generator=gen) - 2))
    if n > 1:
        x[-1] = -x[:-1].double().sum().float()
    return x


def ce_inputs(rows, C, ignore_index):
    """per row an offset from {-300, 0, 300} plus N(0, 30^2).  With >= 7 rows: row 0 equal logits; row 1 has -inf in two non-label columns (C >= 3); rows 2 / 3
    are labelled 0 / C - 1; row 4 carries ignore_index, rows 5 / 6 the labels C and C + 7 (ignored as well)."""
    gen = _gen(6, rows, C, ignore_index)
    off = torch.tensor([-300.0, 0.0, 300.0])[torch.randint(0, 3, (rows,), generator=gen)].unsqueeze(1)
    logits = off + 30 * torch.randn(rows, C, generator=gen, dtype=F32)
    labels = torch.randint(0, C, (rows,), generator=gen, dtype=torch.int64)
    if rows >= 7:
        logits[0] = 7.25
        if C >= 3:
            labels[1] = 1
            logits[1, 0] = logits[1, C - 1] = -math.inf
        labels[2], labels[3], labels[4], labels[5], labels[6] = 0, C - 1, ignore_index, C, C + 7
    return dict(logits=logits, labels=labels)


# ------------------------------------------------------------------------------------------------ every compared quantity of a case, one precision against float64
def cast(d, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in d.items()}


def ln_fwd_dev(case, dtype=F32, mutant=None):
    """{quantity: ratio-to-scale of `dtype` against float64} for one forward case"""
    rows, D, xb = case[:3]
    i = ln_inputs(rows, D, xb)
    a, w = (layer_norm_fwd(cast(i, t)['x'], cast(i, t)['gamma'], mutant=m) for t, m in ((dtype, mutant), (F64, None)))
    return dict(ln_y=ratio(a['y'], w['y'], w['y_scale']), ln_mean=ratio(a['mean'], w['mean'], w['mean_scale']), ln_rstd=ratio(a['rstd'], w['rstd'], w['rstd']))


def ln_bwd_dev(case, dtype=F32):
    rows, D, _, xb, _, ex = case[:6]
    i = ln_inputs(rows, D, xb)
    st = layer_norm_fwd(i['x'].double(), i['gamma'].double())
    mean, rstd = st['mean'].float(), st['rstd'].float()                        # the statistics the kernel is fed: float64, rounded to fp32
    a, w = (layer_norm_bwd(c['dy'], c['x'], mean.to(t), rstd.to(t), c['gamma'], c['extra'] if ex else None) for t in (dtype, F64) for c in (cast(i, t),))
    return dict(ln_dx=ratio(a['dx'], w['dx'], w['dx_scale']), ln_dgamma=ratio(a['dgamma'], w['dgamma'], w['dgamma_scale']))


def geglu_fwd_dev(case, dtype=F32, mutant=None):
    rows, I, Ipad = case[:3]
    i = geglu_inputs(rows, I)
    a, w = (geglu_ln_fwd(c['ux'], c['ug'], c['gamma'], mutant=m, Ipad=Ipad) for t, m in ((dtype, mutant), (F64, None)) for c in (cast(i, t),))
    return dict(gl_hn=ratio(a['hn'], w['hn'], w['hn_scale']), gl_mean=ratio(a['mean'], w['mean'], w['mean_scale']), gl_rstd=ratio(a['rstd'], w['rstd'], w['rstd']))


def geglu_bwd_dev(case, dtype=F32, mutant=None):
    rows, I, Ipad = case[:3]
    i = geglu_inputs(rows, I)
    st = geglu_ln_fwd(i['ux'].double(), i['ug'].double(), i['gamma'].double())
    mean, rstd = st['mean'].float(), st['rstd'].float()
    a, w = (geglu_ln_bwd(c['dhn'], c['ux'], c['ug'], c['gamma'], mean.to(t), rstd.to(t), mutant=m) for t, m in ((dtype, mutant), (F64, None))
            for c in (cast(i, t),))
    return dict(gl_du=max(ratio(a['dux'], w['dux'], w['du_scale']), ratio(a['dug'], w['dug'], w['du_scale'])),
                gl_dgamma=ratio(a['dgamma'], w['dgamma'], w['dgamma_scale']))


def geglu_plain_dev(case, dtype=F32):
    i = geglu_plain_inputs(*case)
    (ya, _), (yw, ys) = (geglu_fwd(i['x'].to(t)) for t in (dtype, F64))
    (da, _), (dw, ds) = (geglu_bwd(i['dy'].to(t), i['x'].to(t)) for t in (dtype, F64))
    return dict(ge_y=ratio(ya, yw, ys), ge_dx=ratio(da, dw, ds))


def colsum_dev(case, dtype=F32):
    rows, cols, bf, scale, acc = case
    i = colsum_inputs(rows, cols, bf)
    (a, _), (w, s) = (colsum(i['x'].to(t), scale, i['prev'].to(t) if acc else None) for t in (dtype, F64))
    return dict(colsum=ratio(a, w, s))


def reduce_dev(n, dtype=F32):
    x = reduce_inputs(n)
    (a, _), (w, s) = (reduce_sum(x.to(t), 0.37) for t in (dtype, F64))
    return dict(reduce_sum=ratio(a, w, s))


def ce_dev(case, dtype=F32, mutant=None):
    rows, C, ign, gs = case
    i = ce_inputs(rows, C, ign)
    lab = i['labels']
    a, w = (cross_entropy_fwd(i['logits'].to(t), lab, ign, mutant=m if m == 'no_max' else None) for t, m in ((dtype, mutant), (F64, None)))
    lse = w['lse'].float()                                                    # the backward is fed the float64 lse rounded to fp32
    da, dw = (cross_entropy_bwd(i['logits'].to(t), lab, lse.to(t), gs, ign, mutant=m) for t, m in ((dtype, mutant), (F64, None)))
    return dict(ce_loss=ratio(a['loss'], w['loss'], w['scale']), ce_lse=ratio(a['lse'], w['lse'], w['scale']), ce_dlogits=ratio(da, dw, abs(gs)))


def all_deviations(dtype=F32):
    """{quantity: the worst deviation over the whole case matrix}: what TOL is ten times of"""
    dev = {}

    def up(d):
        for k, v in d.items():
            dev[k] = max(dev.get(k, 0.0), v)
    for c in ln_fwd_cases():
        up(ln_fwd_dev(c, dtype))
    for c in ln_bwd_cases():
        up(ln_bwd_dev(c, dtype))
    for c in geglu_cases('fwd'):
        up(geglu_fwd_dev(c, dtype))
    for c in geglu_cases('bwd'):
        up(geglu_bwd_dev(c, dtype))
    for c in GEGLU_PLAIN:
        up(geglu_plain_dev(c, dtype))
    for c in colsum_cases():
        up(colsum_dev(c, dtype))
    for n in REDUCE_NS:
        up(reduce_dev(n, dtype))
    for c in ce_cases():
        up(ce_dev(c, dtype))
    return dev
