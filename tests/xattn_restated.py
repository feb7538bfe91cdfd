"""Plain-torch restatement of the conditioning-attention pieces (csrc/xattn.hip, audiolm_pytorch_amd/xattn.py), written for this project from the
formulas in the kernels' own comments.  Everything takes its dtype and device from its arguments (float64 in the tests) and nothing here
imports the library under test.

Row layout of the kernels: row r = (b * N + n) * H + h, so per-row tensors are shaped [B, N, H, ...] here (a view of the kernels' [rows][ld]);
the statistics (lse, ndelta) use the flash kernels' [B, H, N].  Attention-level functions use the reference's (b h n d) / (b j d).

  softmax_part / combine / softmax_bwd / delta / dbias : one function per kernel
  joint_attention : ONE softmax over [extra keys | self keys], differentiable -- what the merged forms must equal
  rounded_model   : joint_attention's forward and backward written out, with a bf16 round trip at each of the library's rounding points.  It is
                    the reference side's estimate of the unavoidable error and only sizes the bounds of the composition tests.
"""
import torch

NOT_CAUSAL = None
NEG_INF = float('-inf')


def _visible(B, N, Me, emask, causal_off, device):
    """bool [B, N, 1, Me]: key e visible to query n of batch b iff emask[b, e] and (not causal or e <= n + causal_off)"""
    vis = torch.ones((B, N, 1, Me), dtype=torch.bool, device=device)
    if emask is not None:
        vis = vis & emask.bool()[:, None, None, :]
    if causal_off is not NOT_CAUSAL:
        e, n = torch.arange(Me, device=device), torch.arange(N, device=device)
        vis = vis & (e[None, :] <= n[:, None] + causal_off)[None, :, None, :]
    return vis


def softmax_part(S, scale, emask=None, lse_self=None, bias=None, causal_off=NOT_CAUSAL):
    """S [B, N, H, Me] raw scores; emask [B, Me] (True = attend) | None; lse_self [B, H, N] | None; bias [H, N, Me] | None, added to the scaled scores;
    causal_off: key e visible to query n iff e <= n + causal_off (NOT_CAUSAL: every key).
    -> (P [B, N, H, Me] = exp(score - lse_tot) on visible keys and 0 elsewhere, lse_tot [B, H, N] = logaddexp(lse_self, lse_e),
        fself [B, N, H] = exp(lse_self - lse_tot)).  A row with no visible key and no self part: P = 0, lse_tot = -inf, fself = 0.
    Hidden positions of S / bias are never used (they may hold NaN)."""
    B, N, H, Me = S.shape
    vis = _visible(B, N, Me, emask, causal_off, S.device).expand(B, N, H, Me)
    score = S * scale
    if bias is not None:
        score = score + bias.permute(1, 0, 2)[None]
    score = torch.where(vis, score, torch.full_like(score, NEG_INF))
    some = vis.any(-1)
    lse_e = torch.where(some, torch.logsumexp(torch.where(some[..., None], score, torch.zeros_like(score)), -1), torch.full_like(score[..., 0], NEG_INF))
    ls = torch.full_like(lse_e, NEG_INF) if lse_self is None else lse_self.permute(0, 2, 1).to(S.dtype)
    hi, lo = torch.maximum(ls, lse_e), torch.minimum(ls, lse_e)
    alive = hi > NEG_INF
    hi0 = torch.where(alive, hi, torch.zeros_like(hi))
    lt = torch.where(alive, hi0 + torch.log1p(torch.exp(lo - hi0)), hi)       # logaddexp; hi0 is finite, so lo = -inf gives exp(-inf) = 0, never inf - inf
    lt0 = torch.where(alive, lt, torch.zeros_like(lt))
    P = torch.where(vis & alive[..., None], torch.exp(score - lt0[..., None]), torch.zeros_like(score))
    fself = torch.where(alive & (ls > NEG_INF), torch.exp(ls - lt0), torch.zeros_like(ls))
    return P, lt.permute(0, 2, 1), fself


def combine(o_self, fself, o_e):
    """O = fself * O_self + O_e; o_self [T, H, dh] | None (then fself is unused), fself [T, H], o_e [T, H, dh]"""
    return o_e if o_self is None else fself[..., None] * o_self + o_e


def softmax_bwd(P, dP, ndelta, scale):
    """dS = P o (dP + ndelta) * scale; P, dP [B, N, H, Me], ndelta [B, H, N]"""
    return P * (dP + ndelta.permute(0, 2, 1)[..., None]) * scale


def delta(o, dout):
    """ndelta [B, H, N] = -sum_d dO * O; o, dout [B, N, H, dh]"""
    return -(o * dout).sum(-1).permute(0, 2, 1)


def dbias(P, dP, ndelta):
    """dbias [H, N, Me] = sum_b P o (dP + ndelta): the un-scaled dS summed over the batch"""
    return (P * (dP + ndelta.permute(0, 2, 1)[..., None])).sum(0).permute(1, 0, 2)


def _keys(q, k_self, v_self, self_mask, ke, ve, emask, causal_self):
    """-> (k [B, M, dh], v, vis bool [B, 1, N, M], Me) for the key set [extra | self]; the extra keys are visible to every query (subject to emask),
    self key j to query i iff j <= i (causal_self) and self_mask[b, j]"""
    B, _, N, _ = q.shape
    ks, vs, vis, Me = [], [], [], 0
    if ke is not None:
        Me = ke.shape[1]
        ks.append(ke), vs.append(ve)
        m = torch.ones((B, 1, N, Me), dtype=torch.bool, device=q.device)
        vis.append(m if emask is None else m & emask.bool()[:, None, None, :])
    if k_self is not None:
        Ns = k_self.shape[1]
        ks.append(k_self), vs.append(v_self)
        m = torch.ones((B, 1, N, Ns), dtype=torch.bool, device=q.device)
        if self_mask is not None:
            m = m & self_mask.bool()[:, None, None, :]
        if causal_self:
            m = m & torch.ones((N, Ns), dtype=torch.bool, device=q.device).tril(Ns - N)
        vis.append(m)
    return torch.cat(ks, 1), torch.cat(vs, 1), torch.cat(vis, -1), Me


def _scores(q, k, vis, scale, bias):
    """masked scores with hidden entries at -inf (rows with no visible key at 0, flagged by `alive`), and the row log-sum-exp"""
    sim = torch.einsum('bhid,bjd->bhij', q, k) * scale
    if bias is not None:
        sim = sim + bias[None]
    alive = vis.any(-1, keepdim=True)
    sim = torch.where(vis, sim, torch.full_like(sim, NEG_INF))
    sim = torch.where(alive, sim, torch.zeros_like(sim))
    lse = torch.where(alive[..., 0], torch.logsumexp(sim, -1), torch.full_like(sim[..., 0], NEG_INF))
    return sim, alive, lse


def joint_attention(q, k_self, v_self, self_mask, ke, ve, emask, scale, bias=None, causal_self=True, keep=None, p=0., return_lse=False):
    """One softmax over [extra keys | self keys].  q [B, H, N, dh]; k_self / v_self [B, N, dh] | None with self_mask [B, N] | None; ke / ve [B, Me, dh] | None
    with emask [B, Me] | None; bias [H, N, Me + N_self] | None over the whole key set; keep [B, H, N, Me + N_self] 0 / 1 | None: the probabilities are
    multiplied by keep / (1 - p) AFTER the softmax.  A query with no visible key gets a zero output.  -> o [B, H, N, dh] (, lse [B, H, N])"""
    k, v, vis, _ = _keys(q, k_self, v_self, self_mask, ke, ve, emask, causal_self)
    sim, alive, lse = _scores(q, k, vis, scale, bias)
    attn = sim.softmax(-1) * vis
    if keep is not None:
        attn = attn * keep / (1. - p)
    o = torch.einsum('bhij,bjd->bhid', attn, v)
    return (o, lse) if return_lse else o


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def rounded_model(q, k_self, v_self, self_mask, ke, ve, emask, scale, dout, bias=None, causal_self=True, keep=None, p=0., flash_self=True):
    """joint_attention forward AND backward (for the upstream gradient `dout` [B, H, N, dh]) with a bf16 round trip at each of the library's rounding
    points and nothing else:
      xattn.py / xattn.hip : P_e; the combined output O; dS_e; dQ (after the accumulate into the flash kernel's dQ when there is one)
      flash kernels        : their probabilities and dS as bf16 MFMA operands, the output O_self, dQ (before the accumulate)
    Everything between the rounding points is exact (the dtype of the inputs).  flash_self=False: the self keys run through the xattn pieces as well
    (the dense-bias math path: one key set, no flash part).  keep covers the xattn key set only (the flash dropout is not modelled).
    -> dict(o, lse, dq, dke, dve, dk_self, dv_self, dbias); dbias covers the xattn key set, entries that do not apply are None."""
    r = bf16_round
    k, v, vis, Me = _keys(q, k_self, v_self, self_mask, ke, ve, emask, causal_self)
    M = k.shape[1]
    sim, alive, lse = _scores(q, k, vis, scale, bias)
    p_all = sim.softmax(-1) * vis                                    # exp(score - joint lse) on visible keys
    nx = Me if (flash_self and k_self is not None) else M            # columns [0, nx) go through xattn, [nx, M) through the flash kernels
    kx, vx, kf, vf = k[:, :nx], v[:, :nx], k[:, nx:], v[:, nx:]
    assert keep is None or keep.shape[-1] == nx
    P = r(p_all[..., :nx])
    da = 1. / (1. - p) if keep is not None else 1.
    Pd = P if keep is None else P * keep
    o = torch.einsum('bhij,bjd->bhid', Pd, vx) * da
    if nx < M:
        visf = vis[..., nx:]
        af = visf.any(-1, keepdim=True)
        simf = torch.where(af, sim[..., nx:], torch.zeros_like(sim[..., nx:]))
        o_self = r(torch.einsum('bhij,bjd->bhid', r(simf.softmax(-1) * visf), vf))
        lse_self = torch.where(af[..., 0], torch.logsumexp(simf, -1), torch.full_like(lse, NEG_INF))
        fself = torch.where(af[..., 0], torch.exp(lse_self - torch.where(af[..., 0], lse, torch.zeros_like(lse))), torch.zeros_like(lse))
        o = o + fself[..., None] * o_self
    o = r(o)
    nd = -(dout * o).sum(-1, keepdim=True)
    dP = torch.einsum('bhid,bjd->bhij', dout, vx) * da
    if keep is not None:
        dP = dP * keep
    dSu = P * (dP + nd)
    dS = r(dSu * scale)
    dq = torch.einsum('bhij,bjd->bhid', dS, kx)
    dkx, dvx = torch.einsum('bhij,bhid->bjd', dS, q), torch.einsum('bhij,bhid->bjd', Pd, dout) * da
    out = dict(o=o, lse=lse, dbias=dSu.sum(0) if bias is not None else None, dk_self=None, dv_self=None)
    if nx < M:
        pf = p_all[..., nx:]
        dsf = r(pf * (torch.einsum('bhid,bjd->bhij', dout, vf) + nd) * scale)
        dq = r(torch.einsum('bhij,bjd->bhid', dsf, kf)) + dq
        out.update(dk_self=torch.einsum('bhij,bhid->bjd', dsf, q), dv_self=torch.einsum('bhij,bhid->bjd', r(pf), dout))
    elif k_self is not None:
        out.update(dk_self=dkx[:, Me:], dv_self=dvx[:, Me:])
    out.update(dq=r(dq), dke=dkx[:, :Me] if ke is not None else None, dve=dvx[:, :Me] if ke is not None else None)
    return out


# ---------------------------------------------------------------------------------------------- inputs of the composition tests
# (shared by tests/test_xattn_host.py, which proves the formulas on them in float64, and tests/test_gpu_xattn.py, which runs the library on them)

CROSS_CASES = [(2, 37, 3, 1, 64), (1, 1, 8, 7, 64), (2, 200, 8, 65, 64), (3, 33, 6, 130, 64)]          # (B, N, H, Me, dh)
PREFIX_CASES = [(2, 37, 8, 5, 64), (1, 130, 4, 64, 64), (2, 200, 6, 77, 64)]                           # (B, N, H, m, dh)
DENSE_CASES = ['causal', 'causal_prefix', 'noncausal']


def _rn(g, *shape, scale=1.0):
    return bf16_round(torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def extra_mask(B, Me, g, clear_last=True):
    """column 0 stays set (the null key / the first key); with more than one batch row the LAST one has every other column clear (with a single row
    that would leave the case one key wide)"""
    m = torch.rand(B, Me, generator=g) > 0.3
    m[:, 0] = True
    if B > 1 and clear_last:
        m[B - 1, 1:] = False
    return m


def cross_case(B, N, H, Me, dh, seed=0, clear_last=True):
    g = torch.Generator().manual_seed(1000 + seed)
    return dict(q=_rn(g, B, H, N, dh), k_self=None, v_self=None, self_mask=None, ke=_rn(g, B, Me, dh), ve=_rn(g, B, Me, dh), emask=extra_mask(B, Me, g, clear_last),
                bias=None, causal_self=True, flash_self=True, scale=dh ** -0.5, dout=_rn(g, B, H, N, dh))


def prefix_case(B, N, H, m, dh, seed=0):
    """causal self part with a key mask (key 0 kept) + m prefix keys with their own mask; with more than one batch row the last one has its WHOLE prefix
    masked (its result must be the flash kernels' alone)"""
    g = torch.Generator().manual_seed(2000 + seed)
    smask = torch.rand(B, N, generator=g) > 0.2
    smask[:, 0] = True
    pmask = torch.rand(B, m, generator=g) > 0.3
    pmask[0, 0] = True
    if B > 1:
        pmask[B - 1] = False
    return dict(q=_rn(g, B, H, N, dh), k_self=_rn(g, B, N, dh), v_self=_rn(g, B, N, dh), self_mask=smask, ke=_rn(g, B, m, dh), ve=_rn(g, B, m, dh),
                emask=pmask, bias=None, causal_self=True, flash_self=True, scale=dh ** -0.5, dout=_rn(g, B, H, N, dh))


def dense_case(name, seed=0, clear_last=True):
    """the math path with a dense bias: every key runs through the xattn pieces (flash_self=False).  `bias` covers the whole key set; with a prefix its
    first m columns are zeros (the reference pads the bias in front)"""
    g = torch.Generator().manual_seed(3000 + seed)
    if name == 'noncausal':
        B, H, N, dh, Me = 2, 4, 64, 32, 37
        return dict(q=_rn(g, B, H, N, dh), k_self=None, v_self=None, self_mask=None, ke=_rn(g, B, Me, dh), ve=_rn(g, B, Me, dh), emask=extra_mask(B, Me, g, clear_last),
                    bias=_rn(g, H, N, Me).float().double(), causal_self=True, flash_self=False, scale=dh ** -0.5, dout=_rn(g, B, H, N, dh))
    B, H, N, dh = 2, 4, 33, 32
    m = 5 if name == 'causal_prefix' else 0
    smask = torch.rand(B, N, generator=g) > 0.2
    smask[:, 0] = True
    bias = torch.randn(H, N, N, generator=g, dtype=torch.float64).float().double()           # the bias is fp32 in the library
    c = dict(q=_rn(g, B, H, N, dh), k_self=_rn(g, B, N, dh), v_self=_rn(g, B, N, dh), self_mask=smask, ke=None, ve=None, emask=None, bias=bias,
             causal_self=True, flash_self=False, scale=dh ** -0.5, dout=_rn(g, B, H, N, dh))
    if m:
        pmask = torch.rand(B, m, generator=g) > 0.3
        c.update(ke=_rn(g, B, m, dh), ve=_rn(g, B, m, dh), emask=pmask, bias=torch.nn.functional.pad(bias, (m, 0), value=0.))
    return c


def keep_for(c, p, seed=0):
    """seeded 0 / 1 keep mask over the xattn key set of case c, in the reference's (b h n m) layout"""
    M = (0 if c['ke'] is None else c['ke'].shape[1]) + (0 if c['k_self'] is None or c['flash_self'] else c['k_self'].shape[1])
    B, H, N, _ = c['q'].shape
    return (torch.rand(B, H, N, M, generator=torch.Generator().manual_seed(4000 + seed)) >= p).double()


def attention_args(c):
    return (c['q'], c['k_self'], c['v_self'], c['self_mask'], c['ke'], c['ve'], c['emask'], c['scale'])


def relmax(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def relfrob(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def reference(c, keep=None, p=0.):
    """-> dict of o, lse, dq, dke, dve, dk_self, dv_self, dbias from joint_attention and autograd, in the dtype of the case (float64)"""
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('q', 'k_self', 'v_self', 'ke', 've', 'bias') if c[k] is not None}
    g = lambda k: leaves.get(k)
    o, lse = joint_attention(g('q'), g('k_self'), g('v_self'), c['self_mask'], g('ke'), g('ve'), c['emask'], c['scale'], bias=g('bias'),
                             causal_self=c['causal_self'], keep=keep, p=p, return_lse=True)
    o.backward(c['dout'])
    grad = lambda k: None if g(k) is None else g(k).grad
    ref = dict(o=o.detach(), lse=lse.detach(), dq=grad('q'), dke=grad('ke'), dve=grad('ve'), dk_self=grad('k_self'), dv_self=grad('v_self'), dbias=grad('bias'))
    return ref


def model_and_reference(c, keep=None, p=0.):
    """-> (ref, model): reference(c) and rounded_model on the same inputs"""
    model = rounded_model(*attention_args(c), c['dout'], bias=c['bias'], causal_self=c['causal_self'], keep=keep, p=p, flash_self=c['flash_self'])
    return reference(c, keep, p), model


def term_magnitudes(c, keep=None, p=0.):
    """every compared quantity of case c recomputed with the ABSOLUTE value of each term (probabilities are positive; |dP| = |dO| |V|^T, |delta| = sum |dO o O|):
    the scale that fp32 accumulation errors are relative to.  Where the terms cancel (one visible key: dS = P (dP - delta) = 0) the result itself is no scale."""
    k, v, vis, Me = _keys(*attention_args(c)[:7], c['causal_self'])
    q, dout, scale = c['q'], c['dout'], c['scale']
    sim, alive, lse = _scores(q, k, vis, scale, c['bias'])
    P = sim.softmax(-1) * vis
    nx = Me if (c['flash_self'] and c['k_self'] is not None) else k.shape[1]
    da = 1. / (1. - p) if keep is not None else 1.
    kp = torch.ones_like(P)
    if keep is not None:
        kp[..., :nx] = keep * da
    Pd = P * kp
    o = torch.einsum('bhij,bjd->bhid', Pd, v.abs())
    A = P * (torch.einsum('bhid,bjd->bhij', dout.abs(), v.abs()) * kp + (dout.abs() * o).sum(-1, keepdim=True))
    dk, dv = torch.einsum('bhij,bhid->bjd', A * scale, q.abs()), torch.einsum('bhij,bhid->bjd', Pd, dout.abs())
    has_e, has_s = c['ke'] is not None, c['k_self'] is not None
    return dict(o=o, dq=torch.einsum('bhij,bjd->bhid', A * scale, k.abs()), dke=dk[:, :Me] if has_e else None, dve=dv[:, :Me] if has_e else None,
                dk_self=dk[:, Me:] if has_s else None, dv_self=dv[:, Me:] if has_s else None, dbias=A[..., :nx].sum(0) if c['bias'] is not None else None)
