"""Causal multi-query flash attention (csrc/attention.hip) restated in plain torch from the formulas in the kernels' comments.  Every function takes its
dtype from its arguments (the tests hand it float64) and nothing here imports the library.

Layouts: q, o, dout (b h n d); the single shared k / v head (b n d); mask (b n) bool, True = attend, or None; bias (h n n) in RAW-score units (the
kernels' tbl: added to q.k BEFORE `scale`); keep (b h n n) 0 / 1; lse, delta (b h n).  scale = d^-0.5.

  sim  = scale (q k^T + bias)        key j is visible to query i iff j <= i and mask[b, j]
  P    = softmax over the visible keys, lse = log sum exp; Pt = P keep / (1 - p)        o = Pt v
  delta = sum_d dO O,  dP = dO v^T,  dPt = keep dP / (1 - p),  dS = P o (dPt - delta)
  dQ = scale dS k,  dK = scale dS^T q (summed over the heads),  dV = Pt^T dO,  dtbl[h][s] = scale sum of dS over the pairs that read slot s

DEAD ROWS.  A query with no visible key gets o = 0, lse = -inf, P = 0 and contributes nothing to any gradient: that is this project's contract
(mqa_fwd_kernel `lt > 0.f ? ... : 0`, lse_log2, attn_delta_kernel's nlse = -inf).  The reference fills hidden scores with -finfo.max, which turns such a
row into the uniform average of ALL values; no caller of either ever reads such a row, so the two never meet, and the tests of this file's users pin the
project's version.
"""
import functools

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DH = 64
SCALE = DH ** -0.5
LOG2E = 1.4426950408889634
RESCALE_THR = 8.0                  # log2 units (attention.hip)
M32 = 0xffffffff
U = 2.0 ** -8                      # unit roundoff of bf16 (8-bit significand): the worst case of one round-to-nearest, reached just above a power of two


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf(t):
    """one bf16 round trip"""
    return t.to(F32).to(BF16).to(t.dtype)


def randbf(g, *shape, scale=1.):
    return (torch.randn(*shape, generator=g) * scale).to(BF16).double()


# ------------------------------------------------------------------------------------------------ forward / backward

def visible(B, N, mask):
    """(b 1 n n) bool: key j visible to query i"""
    vis = torch.ones(N, N, dtype=torch.bool).tril()[None, None]
    if mask is not None:
        vis = vis & mask[:, None, None, :]
    return vis.expand(B, 1, N, N)


def sim(q, k, scale, bias=None):
    s = torch.einsum('bhid,bjd->bhij', q, k)
    if bias is not None:
        s = s + bias[None]
    return s * scale


def softmax_rows(S, vis, lse=None):
    """P, lse over the visible keys; a row without one: P = 0, lse = -inf.  With `lse` given P = exp(S - lse) (the backward kernels' form)"""
    S = S.masked_fill(~vis, float('-inf'))
    m = S.amax(-1, keepdim=True)
    live = torch.isfinite(m)
    if lse is None:
        E = torch.exp(S - torch.where(live, m, torch.zeros_like(m)))
        l = E.sum(-1, keepdim=True)
        P = torch.where(live, E / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(E))
        lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float('-inf')))[..., 0]
    else:
        dead = torch.isinf(lse)[..., None]
        P = torch.where(dead, torch.zeros_like(S), torch.exp(S - torch.where(dead, torch.zeros_like(S[..., :1]), lse[..., None].to(S.dtype))))
    return P, lse


def attention(q, k, v, mask, scale, bias=None, keep=None, p=0.):
    """-> (o, lse, P); P is the softmax BEFORE dropout (dropped pairs count in the normalisation: dropout acts on the softmax output)"""
    B, H, N, _ = q.shape
    P, lse = softmax_rows(sim(q, k, scale, bias), visible(B, N, mask))
    Pt = P if keep is None else P * keep / (1. - p)
    return torch.einsum('bhij,bjd->bhid', Pt, v), lse, P


def backward(q, k, v, mask, scale, dout, bias=None, keep=None, p=0., o=None, lse=None, slot=None, LT=0, delta_=None):
    """-> dict(dq, dk, dv, delta[, dtbl]); o / lse: the forward's (recomputed when None; delta_ overrides sum_d dO O).  slot (n n) long: table slot each pair reads, -1 = none"""
    B, H, N, _ = q.shape
    vis = visible(B, N, mask)
    if o is None or lse is None:
        o, lse, _ = attention(q, k, v, mask, scale, bias, keep, p)
    P, _ = softmax_rows(sim(q, k, scale, bias), vis, lse)
    kp = 1. if keep is None else keep / (1. - p)
    dl = (dout * o).sum(-1) if delta_ is None else delta_
    dl = torch.where(torch.isinf(lse), torch.zeros_like(dl), dl)
    dS = P * (torch.einsum('bhid,bjd->bhij', dout, v) * kp - dl[..., None])
    out = dict(dq=scale * torch.einsum('bhij,bjd->bhid', dS, k), dk=scale * torch.einsum('bhij,bhid->bjd', dS, q),
               dv=torch.einsum('bhij,bhid->bjd', P * kp, dout), delta=dl)
    if slot is not None:
        out['dtbl'] = table_grad(dS, slot, LT, scale)
    return out


def table_grad(dS, slot, LT, scale):
    H = dS.shape[1]
    ok = (slot >= 0).flatten()
    d = torch.zeros(H, LT, dtype=dS.dtype)
    d.index_add_(1, slot.flatten()[ok], dS.sum(0).reshape(H, -1)[:, ok])
    return d * scale


def delta(o, dout, lse, scale):
    """what attn_delta_kernel writes: ndelta = -sum_d dO O, nlse = -lse / scale (-inf stays -inf: every P of that row is exp2(-inf) = 0)"""
    nd = -(dout * o).sum(-1)
    nl = torch.where(torch.isinf(lse), torch.full_like(lse, float('-inf')), -lse / scale)
    return nd, nl


def kv_grad_pack(parts, acc, mode, skip=None):
    """parts (g rows 2d) fp32 partial (dk | dv) sets -> (dkv rounded once to bf16, acc afterwards).  mode 0: no value residual; 1: this layer's v was
    mixed, half of dv goes to layer 0's accumulator; 2: layer 0 receives the accumulator.  skip: a partial set left out (the mutant)"""
    d = parts.shape[-1] // 2
    s = sum(parts[i] for i in range(parts.shape[0]) if i != skip)
    gk, gv = s[:, :d], s[:, d:]
    if mode == 1:
        gv = 0.5 * gv
        acc = acc + gv
    elif mode == 2:
        gv = gv + acc
    return torch.cat((gk, gv), 1), acc


# ------------------------------------------------------------------------------------------------ dropout hash

def mix32(x):
    x = x & M32
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & M32          # (int64 tensors wrap: the low 32 bits survive)
    return x ^ (x >> 16)


def drop_salt(seed, b, h, H):
    lo, hi = seed & M32, (seed >> 32) & M32
    return mix32(lo ^ mix32((hi + (b * H + h) * 0x9E3779B9) & M32))


def drop_thr(p):
    return min(int(p * 4294967296.0), 4294967295)


def drop_keep(seed, b, h, i, j, N, H, thr):
    """pair (i, j) of (b, h) is kept iff mix32((i N + j) ^ salt) >= thr; i, j int64 tensors"""
    return mix32(((i * N + j) & M32) ^ drop_salt(seed, b, h, H)) >= thr


def keep_mask(seed, B, H, N, p, dtype=F64):
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    return torch.stack([torch.stack([drop_keep(seed, b, h, i, j, N, H, drop_thr(p)) for h in range(H)]) for b in range(B)]).to(dtype)


# ------------------------------------------------------------------------------------------------ structured bias (relpos.toeplitz_index restated)

def toeplitz_index(N, num_leading=None):
    pos = torch.arange(N)
    qkey4, kkey4 = (4 * (pos + N)).int(), (4 * pos).int()
    if num_leading is None:
        return qkey4, kkey4, torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    return qkey4, kkey4, (pos >= num_leading).int(), (pos < num_leading).int()


def dense_bias(tbl, index):
    """-> (bias (h n n) raw-score units, slot (n n) long, -1 where the offset falls outside the table and reads 0)"""
    qkey4, kkey4, qattr, kattr = [t.long() for t in index]
    LT = tbl.shape[1]
    off = qkey4[:, None] - kkey4[None, :]
    special = (qattr[:, None] & kattr[None, :]) != 0
    slot = torch.where(special, torch.zeros_like(off), torch.where((off >= 0) & (off < 4 * LT), off // 4, torch.full_like(off, -1)))
    vals = torch.where((slot >= 0)[None], tbl[:, slot.clamp(min=0)], torch.zeros((), dtype=tbl.dtype))
    return vals, slot


# ------------------------------------------------------------------------------------------------ the kernels' tile loop (branch census, alpha mutant)

def online_forward(q, k, v, mask, scale, skip_rescale=False):
    """mqa_fwd_kernel<QB = 1>'s online softmax in exact arithmetic: 32-query blocks, 64-key tiles, the running maximum m (log2 units) raised -- for the
    WHOLE block, `__any(need)` -- only when some row's tile maximum exceeds its m by more than RESCALE_THR.  -> (o, lse, census): census counts, per (row,
    tile) with a visible key, 'raise' (tm > m + thr), 'defer' (m < tm <= m + thr and the block did not rescale: P up to 2^thr against a stale m) and 'keep'
    (tm <= m).  skip_rescale: alpha = 1 (the mutant: m moves, o and l are not rescaled)."""
    B, H, N, D = q.shape
    c2 = scale * LOG2E
    S = sim(q, k, 1.).masked_fill(~visible(B, N, mask), float('-inf'))
    o, lse = torch.zeros_like(q), torch.full((B, H, N), float('-inf'), dtype=q.dtype)
    census = dict.fromkeys(('raise', 'defer', 'keep'), 0)
    for q0 in range(0, N, 32):
        q1 = min(q0 + 32, N)
        m = torch.full((B, H, q1 - q0), float('-inf'), dtype=q.dtype)
        l, acc = torch.zeros_like(m), torch.zeros((B, H, q1 - q0, D), dtype=q.dtype)
        for t0 in range(0, q1, 64):
            st = S[:, :, q0:q1, t0:t0 + 64]
            tm = st.amax(-1) * c2
            need = tm > m + RESCALE_THR
            any_need = need.flatten(2).any(-1)[..., None]                                    # one wave = one (b, h, block)
            has = torch.isfinite(tm)
            census['raise'] += int((need & has).sum())
            census['defer'] += int((has & ~any_need & (tm > m) & torch.isfinite(m)).sum())
            census['keep'] += int((has & (tm <= m)).sum())
            mn = torch.where(any_need, torch.maximum(m, tm), m)
            alpha = torch.where(torch.isinf(mn), torch.ones_like(m), torch.exp2(torch.where(torch.isinf(mn), torch.zeros_like(m), m - mn)))
            if skip_rescale:
                alpha = torch.ones_like(alpha)
            m, l, acc = mn, l * alpha, acc * alpha[..., None]
            pv = torch.exp2(st * c2 - torch.where(torch.isinf(m), torch.zeros_like(m), m)[..., None])
            l = l + pv.sum(-1)
            acc = acc + torch.einsum('bhij,bjd->bhid', pv, v[:, t0:t0 + 64])
        live = l > 0
        inv = torch.where(live, 1. / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(l))
        o[:, :, q0:q1] = acc * inv[..., None]
        lse[:, :, q0:q1] = torch.where(live, m / LOG2E + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(l, float('-inf')))
    return o, lse, census


# ------------------------------------------------------------------------------------------------ rounded model and term sums (they only size bounds)

def rounded_model(q, k, v, mask, scale, dout, bias=None, keep=None, p=0., slot=None, LT=0):
    """the same forward and backward with a bf16 round trip at every point where the kernels round:
    forward: P (un-normalised, after the keep mask) before the second MFMA; O on store.   delta: reads the stored (rounded) O.
    backward: P (after keep) before the dV MFMA, dS before the dQ and dK MFMAs, dQ on store.  lse, delta, dK, dV, dtbl stay fp32 (here: exact)."""
    B, H, N, _ = q.shape
    vis = visible(B, N, mask)
    S = sim(q, k, scale, bias).masked_fill(~vis, float('-inf'))
    m = S.amax(-1, keepdim=True)
    live = torch.isfinite(m)
    E = torch.exp(S - torch.where(live, m, torch.zeros_like(m)))
    l = torch.where(live, E.sum(-1, keepdim=True), torch.ones_like(m))
    kp = 1. if keep is None else keep
    o = bf(torch.einsum('bhij,bjd->bhid', bf(E * kp), v) / l / (1. - p))
    o = torch.where(live, o, torch.zeros_like(o))
    lse = torch.where(live, m + torch.log(l), torch.full_like(m, float('-inf')))[..., 0]
    P, _ = softmax_rows(S, vis, lse)
    dl = torch.where(torch.isinf(lse), torch.zeros_like(lse), (dout * o).sum(-1))
    dSf = P * (torch.einsum('bhid,bjd->bhij', dout, v) * kp / (1. - p) - dl[..., None])
    dS = bf(dSf)
    out = dict(o=o, lse=lse, dq=bf(scale * torch.einsum('bhij,bjd->bhid', dS, k)), dk=scale * torch.einsum('bhij,bhid->bjd', dS, q),
               dv=torch.einsum('bhij,bhid->bjd', bf(P * kp), dout) / (1. - p))
    if slot is not None:
        out['dtbl'] = table_grad(dSf, slot, LT, scale)              # the table gradient takes the fp32 dS (before the bf16 pack)
    return out


def term_sums(q, k, v, mask, scale, dout, bias=None, keep=None, p=0., slot=None, LT=0):
    """per-element sums of ABSOLUTE terms, the scale of each element's rounding error:
      o   sum_j Pt |v|            dv  sum_{h,i} Pt |dO|          tdelta = sum_d |dO O|  (>= |delta|)
      dq  scale sum_j P (|dPt| + tdelta) |k|       dk  scale sum_{h,i} P (|dPt| + tdelta) |q|
      dtbl  scale sum_{pairs of the slot} P tdelta (the table gradient takes the fp32 dS: the rounded O inside delta is its only bf16 point)
      dtbl_f  scale sum_{pairs} P (sum_d |dO| |v| keep / (1 - p) + tdelta): the scale of the fp32 dot products behind dS
      dtbl_q  scale * (pairs of the slot) * max over the head of P (|dPt| + |delta|): the scale of the dQ kernel's block-scaled integer quantisation"""
    B, H, N, _ = q.shape
    o, lse, P = attention(q, k, v, mask, scale, bias, keep, p)
    kp = 1. if keep is None else keep / (1. - p)
    Pt = P * kp
    td = torch.where(torch.isinf(lse), torch.zeros_like(lse), (dout * o).abs().sum(-1))
    dl = torch.where(torch.isinf(lse), torch.zeros_like(lse), (dout * o).sum(-1))
    dPt = (torch.einsum('bhid,bjd->bhij', dout, v) * kp).abs()
    A = P * (dPt + td[..., None])
    out = dict(o=torch.einsum('bhij,bjd->bhid', Pt, v.abs()), dv=torch.einsum('bhij,bhid->bjd', Pt, dout.abs()), tdelta=td,
               dq=scale * torch.einsum('bhij,bjd->bhid', A, k.abs()), dk=scale * torch.einsum('bhij,bhid->bjd', A, q.abs()),
               smax=(sim(q, k, scale, bias).abs() * visible(B, N, mask)).amax(-1))
    if slot is not None:
        out['dtbl'] = table_grad(P * td[..., None], slot, LT, scale)
        out['dtbl_f'] = table_grad(P * (torch.einsum('bhid,bjd->bhij', dout.abs(), v.abs()) * kp + td[..., None]), slot, LT, scale)
        cnt = table_grad((P > 0).to(q.dtype), slot, LT, 1.)
        out['dtbl_q'] = scale * cnt * (P * (dPt + dl.abs()[..., None])).amax((0, 2, 3))[:, None]
    return out


# first-order worst case of each output: (number of bf16 rounding points that reach it) x U x its term sum -- derivation in tests/test_attn_host.py
WORST = dict(o=2 * U, dq=3 * U, dk=2 * U, dv=1 * U, dtbl=1 * U)
BOUND = {k_: 2 * w for k_, w in WORST.items()}                      # the tests' element-wise bounds: twice the worst case
QUANT = 2.0 ** -19                                                  # dtbl: one addend's integer quantisation, relative to the pass maximum of |dS|
F32_DOT = 2.0 ** -16                                               # dtbl: 64-term fp32 dot products and <= 2^15 fp32 addends per slot, relative to their absolute terms
LSE_ABS, LSE_REL = 1e-4, 8 * 2.0 ** -24                             # |d lse| <= 1e-4 + 8 u32 max_j |sim|


def bounds(T):
    """element-wise bounds from term_sums"""
    b = {n: BOUND[n] * T[n] for n in ('o', 'dq', 'dk', 'dv')}
    b['lse'] = LSE_ABS + LSE_REL * T['smax']
    if 'dtbl' in T:
        b['dtbl'] = BOUND['dtbl'] * T['dtbl'] + 2 * (F32_DOT * T['dtbl_f'] + QUANT * T['dtbl_q'])
    return b


def ratio(got, want, bound):
    """max over the elements of |got - want| / bound; an element whose bound is 0 (dead row, masked key) has to be exact: any error there counts as inf"""
    err = (got - want).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.


# ------------------------------------------------------------------------------------------------ input builders (seeded, every value exact in bf16)

def random_inputs(B, N, H, masked, g):
    mask = (torch.rand(B, N, generator=g) > 0.25) if masked else None
    return dict(q=randbf(g, B, H, N, DH), k=randbf(g, B, N, DH), v=randbf(g, B, N, DH), dout=randbf(g, B, H, N, DH), mask=mask)


def needle(N, H, mask, g, B=None):
    """k_j random +-1 vectors; query (i, h) is 8 k_t with t = t(b, h, i) drawn from the keys visible to i (a query without one is 0, target -1): the target
    scores 8 * 64 / 8 = 64 nats, any other key 64 minus twice the number of differing signs, so P is the one-hot of t far below fp32 resolution and
    o = v[t] EXACTLY.  The queries N - 1, N - 2, ... of head 0 are pointed at the tile-boundary keys 64, 128, ... (where visible): a key lost at a tile
    edge is then some query's whole answer."""
    B = mask.shape[0] if mask is not None else (B or 1)
    k = (torch.randint(0, 2, (B, N, DH), generator=g) * 2 - 1).double()
    vis = visible(B, N, mask)[:, 0]                                                    # b i j
    w = torch.rand(B, H, N, N, generator=g) * vis[:, None]
    tgt = torch.where(vis.any(-1)[:, None], w.argmax(-1), torch.full((B, H, N), -1))
    for tt in range(1, (N - 1) // 64 + 1):
        i, j = N - tt, 64 * tt
        if i > j:
            tgt[:, 0, i] = torch.where(vis[:, i, j], torch.full((B,), j), tgt[:, 0, i])
    q = torch.where((tgt >= 0)[..., None], 8. * torch.gather(k[:, None].expand(B, H, N, DH), 2, tgt.clamp(min=0)[..., None].expand(B, H, N, DH)), torch.zeros(()).double())
    return dict(q=q, k=k, v=randbf(g, B, N, DH), dout=randbf(g, B, H, N, DH), mask=mask, target=tgt)


def ramp(N, slope, g, B=1, H=1):
    """scores that climb with the key index: the first 8 dims of every query hold `slope`, those of key j hold j / 256 (exact in bf16 for j <= 256), so
    sim(i, j) = slope j / 256 nats for every query; the other 56 dims are N(0, 1) on both sides (+- ~1 nat of noise, so that rows differ).
      slope +28: 0.109 nats / key, 7 nats = 10.1 log2 units per 64-key tile: every tile's maximum beats the running one by more than 8 -> raise every tile
      slope +10: 0.039 nats / key, 3.6 log2 units per tile: m stays stale for two tiles (P up to ~2^7.2), then is raised
      slope -28: the first tile holds the maximum, m never moves, later P fall to e^-28
    |sim| <= 28 + noise: far inside 60 nats."""
    assert N <= 257
    q, k = randbf(g, B, H, N, DH), randbf(g, B, N, DH)
    q[..., :8] = float(slope)
    k[..., :8] = (torch.arange(N).double() / 256.)[None, :, None]
    return dict(q=q, k=k, v=randbf(g, B, N, DH), dout=randbf(g, B, H, N, DH), mask=None)


PREFIX_LENGTHS = (1, 31, 32, 33, 64, 65)


def masked_prefix(B, N, lengths):
    """mask (b n): row r < len(lengths) has its first lengths[r] keys masked (its queries before that are dead rows), then one row with EVERY key masked,
    then one without a mask"""
    assert B == len(lengths) + 2 and all(0 < L < N for L in lengths)
    mask = torch.ones(B, N, dtype=torch.bool)
    for r, L in enumerate(lengths):
        mask[r, :L] = False
    mask[B - 2] = False
    return mask


def prefix_inputs(N, H, g):
    lengths = tuple(L for L in PREFIX_LENGTHS if L < N - 1) + (N - 1,)
    B = len(lengths) + 2
    d = random_inputs(B, N, H, False, g)
    d['mask'] = masked_prefix(B, N, lengths)
    return d


# ------------------------------------------------------------------------------------------------ the cases shared by the host and the GPU test

NS = (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200, 257)
# random inputs: every N once, H in {1, 3, 4, 5, 8} (inactive waves: 1, 3, 5; a second head group: 5, 8), B in {1, 2, 3}; odd entries carry a 25 % key mask
RANDOM = [(1, 1, 1), (2, 31, 3), (1, 32, 4), (3, 33, 5), (1, 63, 8), (2, 64, 1), (1, 65, 3), (2, 96, 4), (1, 127, 5), (2, 128, 8), (3, 129, 3), (2, 200, 5), (1, 257, 8),
          (4, 129, 8)]      # B x HG = 8 with 3 (dQ, dK/dV) / 3 (forward pairs) blocks: decode_block's XCD branches with an odd block count
RAMPS = {'ramp-raise': (257, 28, 1, 3), 'ramp-stale': (200, 10, 2, 4), 'ramp-neg': (257, -28, 1, 5)}          # N, slope, B, H
NEEDLES = [(N, (1, 3, 4, 5, 8)[i % 5], 1 + i % 2) for i, N in enumerate(NS)]                                 # N, H, B
PREFIX = (129, 5)                                                                                             # N, H (B = 9 rows)
VARIANTS = [(kind, p) for kind in (None, 'toeplitz', 'coarse') for p in (0., 0.25) if kind or p]              # the bias / dropout instantiations
SEED = 0x1234_5678_9abc_def


def case_names():
    names = [f'rand-{B}x{N}x{H}' + ('-m' if i % 2 else '') for i, (B, N, H) in enumerate(RANDOM)]
    names += list(RAMPS) + ['prefix'] + [f'needle-{N}' + s for N, _, _ in NEEDLES for s in ('', '-m')]
    return names


def variant_names():
    return [f'{base}+{kind or "nobias"}+p{p}' for base in ('prefix', 'ramp-raise') for kind, p in VARIANTS]


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one named case (float64, every value exact in bf16; tbl exact in fp32), built once"""
    base, *var = name.split('+')
    g = gen(sum(ord(c) * (i + 1) for i, c in enumerate(base)))
    if base.startswith('rand-'):
        B, N, H = (int(x) for x in base.split('-')[1].split('x'))
        c = random_inputs(B, N, H, base.endswith('-m'), g)
    elif base in RAMPS:
        N, slope, B, H = RAMPS[base]
        c = ramp(N, slope, g, B, H)
    elif base == 'prefix':
        c = prefix_inputs(*PREFIX, g)
    else:
        N = int(base.split('-')[1])
        _, H, B = next(x for x in NEEDLES if x[0] == N)
        c = needle(N, H, (torch.rand(B, N, generator=g) > 0.25) if base.endswith('-m') else None, g, B=B)
    c.update(scale=SCALE, bias=None, keep=None, p=0., slot=None, LT=0, tbl=None, index=None, name=name)
    if var:
        kind, p = var[0], float(var[1][1:])
        B, H, N, _ = c['q'].shape
        if kind != 'nobias':
            c['index'] = toeplitz_index(N, N // 3 + 1 if kind == 'coarse' else None)
            c['LT'] = 2 * N
            c['tbl'] = (torch.randn(H, 2 * N, generator=g) * 16.).float().double()           # raw-score units: +- 2 nats after the scale
            c['bias'], c['slot'] = dense_bias(c['tbl'], c['index'])
        if p:
            c['p'], c['keep'] = p, keep_mask(SEED, B, H, N, p)
    return c


ARGS = ('q', 'k', 'v', 'mask', 'scale')
KW = ('bias', 'keep', 'p')


def fwd_args(c):
    return [c[a] for a in ARGS], {a: c[a] for a in KW}


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 restatement, term sums and bounds of one case, computed once and shared"""
    c = case(name)
    a, kw = fwd_args(c)
    o, lse, P = attention(*a, **kw)
    ref = backward(*a, c['dout'], **kw, o=o, lse=lse, slot=c['slot'], LT=c['LT'])
    ref.update(o=o, lse=lse)
    T = term_sums(*a, c['dout'], **kw, slot=c['slot'], LT=c['LT'])
    return ref, T, bounds(T)


def model(name):
    c = case(name)
    a, kw = fwd_args(c)
    return rounded_model(*a, c['dout'], **kw, slot=c['slot'], LT=c['LT'])


def needle_margins(c):
    """(smallest margin in nats between the target and any other visible key, largest off-target probability mass) over the live queries"""
    B, H, N, _ = c['q'].shape
    S = sim(c['q'], c['k'], c['scale']).masked_fill(~visible(B, N, c['mask']), float('-inf'))
    live = c['target'] >= 0
    t = c['target'].clamp(min=0)[..., None]
    top = torch.gather(S, 3, t)[..., 0]
    rest = S.scatter(3, t, float('-inf')).amax(-1)
    P, _ = softmax_rows(S, visible(B, N, c['mask']))
    off = 1. - torch.gather(P, 3, t)[..., 0]
    return float((top - rest)[live].min()), float(off[live].max()), float((top[live] - 64.).abs().max())
