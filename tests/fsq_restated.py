"""TEST INFRASTRUCTURE ONLY.  Plain-torch restatement of finite scalar quantization (FSQ, arXiv 2309.15505, Appendix A) in the residual, grouped form
of vector-quantize-pytorch's `GroupedResidualFSQ` as the reference builds it (audiolm_pytorch/soundstream.py:578-586).  Runs on the CPU in float64
or float32; gradients come from torch autograd of this forward (straight-through rounding, detached residual update), never from hand-written
formulas -- `closed_form_dz` below is the formula the kernels implement, and tests/test_fsq_host.py checks it against that autograd.

THIS IS A RESTATEMENT, PARITY UNPINNED: the upstream library is not vendored and no golden vectors of it exist here.  The arithmetic below is this
project's specification; where a detail of the upstream library differs, this text wins.  The three places where the paper and the package are known
to differ are the three constants right below the imports, so that a later check against the installed package is a one-line change each.

  per group (features chunked along the last dim), levels L (d entries), Q quantizers:
    half_l  = (L - 1) * (1 + HALF_L_SIGN * EPS) / 2          offset = 0.5 where L is even, else 0
    shift   = atanh(offset / half_l)                          half_w = L // 2
    basis   = cumprod([1, L[0], ..., L[d-2]])                 scale_q = (L - 1) ** (-q)  per dimension, q = 0 .. Q-1
    z = project_in(x)  (nn.Linear(dim_g, d); identity when dim_g == d) ; r_0 = z
    for q in 0 .. k (k = last active layer: quantize dropout in training, Q - 1 in eval):
        b_q = tanh(r_q / scale_q + shift) * half_l - offset
        c_q = round_half_even(b_q)                            straight-through: d c_q / d b_q = 1
        idx_q = sum_j (c_q[j] + half_w[j]) * basis[j]
        quant_q = c_q / half_w * scale_q ;  r_{q+1} = r_q - quant_q.detach()
    out = project_out(sum_q quant_q)  (nn.Linear(d, dim_g) or identity) ; indices of dropped layers (q > k) are -1
  decode: c = idx // basis % L - half_w ; sum over the given columns of c / half_w * scale_q (-1 contributes zero) ; project_out
  dropout index (host): tests/rvq_train_restated.py's dropout_index, one seed per call shared by all groups
"""
from __future__ import annotations

import torch

from rvq_train_restated import dropout_index  # noqa: F401  (the same host rule as the VQ)

EPS = 1e-3
HALF_L_SIGN = +1                     # half_l = (L - 1) * (1 + HALF_L_SIGN * EPS) / 2
SHIFT_FORM = 'atanh'                 # shift = atanh(offset / half_l); 'tan': the paper's listing


def constants(levels, num_quantizers, dtype=torch.float64):
    """dict of half_l, offset, shift, half_w, basis, levels [d] and scale [Q, d] in `dtype`"""
    L = torch.tensor([int(l) for l in levels], dtype=dtype)
    half_l = (L - 1) * (1 + HALF_L_SIGN * EPS) / 2
    offset = torch.where(L % 2 == 0, torch.full_like(L, 0.5), torch.zeros_like(L))
    ratio = offset / half_l
    shift = torch.atanh(ratio) if SHIFT_FORM == 'atanh' else torch.tan(ratio)
    half_w = torch.floor(L / 2)
    basis = torch.cumprod(torch.cat([torch.ones(1, dtype=dtype), L[:-1]]), dim=0)
    q = torch.arange(num_quantizers, dtype=dtype)
    scale = (L - 1)[None, :] ** (-q)[:, None]
    return dict(levels=L, half_l=half_l, offset=offset, shift=shift, half_w=half_w, basis=basis, scale=scale)


def bound(r, c, q):
    return torch.tanh(r / c['scale'][q] + c['shift']) * c['half_l'] - c['offset']


def round_ste(b):
    return b + (torch.round(b) - b).detach()                 # torch.round: half to even


def codes_to_indices(codes, c):
    """integer-valued codes [..., d] in -half_w .. L - 1 - half_w -> int64 [...]"""
    return ((codes + c['half_w']) * c['basis']).sum(dim=-1).round().to(torch.int64)


def indices_to_codes(idx, c):
    """int64 [...] -> codes [..., d] (the inverse of codes_to_indices)"""
    basis, levels = c['basis'].to(torch.int64), c['levels'].to(torch.int64)
    return ((idx.unsqueeze(-1) // basis) % levels).to(c['half_w'].dtype) - c['half_w']


def residual_chain(z, c, k):
    """z [M, d] -> (zsum [M, d] with the straight-through graph, idx int64 [M, Q] (-1 past k), the pre-rounding b_q [k + 1, M, d] detached)"""
    Q = c['scale'].shape[0]
    r, zsum, inds, bs = z, torch.zeros_like(z), [], []
    for q in range(Q):
        if q > k:
            inds.append(torch.full(z.shape[:-1], -1, dtype=torch.int64))
            continue
        b = bound(r, c, q)
        code = round_ste(b)
        inds.append(codes_to_indices(code.detach(), c))
        quant = code / c['half_w'] * c['scale'][q]
        r = r - quant.detach()
        zsum = zsum + quant
        bs.append(b.detach())
    return zsum, torch.stack(inds, dim=-1), torch.stack(bs)


def closed_form_dz(z, g_z, c, k):
    """the input gradient of residual_chain given g_z = dL/dzsum: the detach() leaves only the direct path of every layer"""
    r, s = z, torch.zeros_like(z)
    for q in range(k + 1):
        t = torch.tanh(r / c['scale'][q] + c['shift'])
        s = s + (c['half_l'] / c['half_w']) * (1 - t ** 2)
        r = r - torch.round(t * c['half_l'] - c['offset']) / c['half_w'] * c['scale'][q]
    return g_z * s


def near_tie(bs, band):
    """bs [k + 1, M, d] -> bool [M]: some |b - floor(b) - 0.5| < band at an active layer"""
    return ((bs - torch.floor(bs) - 0.5).abs() < band).any(dim=-1).any(dim=0)


class GroupFSQ:
    """one group: weights = (W_in [d, dim_g], b_in [d], W_out [dim_g, d], b_out [dim_g]) in the oracle's dtype, or None when dim_g == d"""

    def __init__(self, levels, num_quantizers, weights=None, dtype=torch.float64):
        self.c = constants(levels, num_quantizers, dtype)
        self.d, self.Q, self.dtype = len(levels), num_quantizers, dtype
        self.weights = weights

    def project_in(self, x):
        return x if self.weights is None else x @ self.weights[0].T + self.weights[1]

    def project_out(self, zsum):
        return zsum if self.weights is None else zsum @ self.weights[2].T + self.weights[3]

    def forward(self, x, k=None):
        """x [M, dim_g] -> (out [M, dim_g], idx [M, Q], z [M, d], zsum [M, d], b [k + 1, M, d])"""
        k = self.Q - 1 if k is None else k
        z = self.project_in(x)
        zsum, idx, bs = residual_chain(z, self.c, k)
        return self.project_out(zsum), idx, z, zsum, bs

    def decode(self, idx):
        """idx int64 [M, q <= Q] (-1 = no code) -> out [M, dim_g]"""
        zsum = 0.
        for q in range(idx.shape[-1]):
            col = idx[..., q]
            codes = indices_to_codes(col.clamp(min=0), self.c) / self.c['half_w'] * self.c['scale'][q]
            zsum = zsum + torch.where((col >= 0).unsqueeze(-1), codes, torch.zeros_like(codes))
        return self.project_out(zsum)


class GroupedFSQ:
    """the grouped form: the last axis split into `groups` chunks, outputs concatenated, indices stacked to (g, b, n, q)"""

    def __init__(self, levels, num_quantizers, group_weights, dtype=torch.float64):
        self.groups = [GroupFSQ(levels, num_quantizers, w, dtype) for w in group_weights]

    @classmethod
    def from_module(cls, rq, dtype=torch.float64, requires_grad=False):
        """copies the parameters of a module with the upstream tree (rvqs.{g}.project_in / project_out, nn.Linear or nn.Identity)"""
        ws = []
        for r in rq.rvqs:
            if isinstance(r.project_in, torch.nn.Identity):
                ws.append(None)
            else:
                ws.append(tuple(p.detach().cpu().to(dtype).clone().requires_grad_(requires_grad)
                                for p in (r.project_in.weight, r.project_in.bias, r.project_out.weight, r.project_out.bias)))
        return cls(rq.levels, rq.num_quantizers, ws, dtype)

    def forward(self, x, k=None):
        """x (b, n, dim) -> (out (b, n, dim), indices (g, b, n, Q), near-tie inputs: per group b [k + 1, b n, d])"""
        b, n, _ = x.shape
        outs = [grp.forward(ch.reshape(b * n, -1), k) for grp, ch in zip(self.groups, x.chunk(len(self.groups), dim=-1))]
        return (torch.cat([o[0].reshape(b, n, -1) for o in outs], dim=-1), torch.stack([o[1].reshape(b, n, -1) for o in outs]), [o[4] for o in outs])

    def decode(self, indices):
        g, b, n, q = indices.shape
        return torch.cat([grp.decode(indices[i].reshape(b * n, q)).reshape(b, n, -1) for i, grp in enumerate(self.groups)], dim=-1)
