"""TEST INFRASTRUCTURE ONLY.  Plain-torch restatement of lookup-free quantization (LFQ, arXiv 2310.05737) in the residual, grouped form of
vector-quantize-pytorch's `GroupedResidualLFQ` as the reference builds it (audiolm_pytorch/soundstream.py:563-571).  Runs on the CPU in float64 or
float32.  It is written DENSELY, as the package writes it: the explicit [2^d, d] codebook, an einsum, softmax, the clamped log, the
`x + (quant - x).detach()` straight-through form, and torch autograd for every gradient.  The closed forms the kernels implement (the factorised
log-sum-exp, the losses, dz and the parameter gradients) are SEPARATE helpers at the end; tests/test_lfq_host.py checks them against the dense
formulation and its autograd.

THIS IS A RESTATEMENT, PARITY UNPINNED: the upstream library is not vendored and no golden vectors of it exist here.  The arithmetic below is this
project's specification; where a detail of the upstream library differs, this text wins.

  per group (features chunked along the last dim), d = log2(codebook_size), Q quantizers, M = b n tokens:
    z = project_in(x)  (nn.Linear(dim_g, d); identity when dim_g == d) ; r_0 = z
    for q in 0 .. k (k = last active layer: quantize dropout in training, Q - 1 in eval), s_q = 2^-q:
        bit_q = r_q > 0  (0 counts as not set) ;  quant_q = where(bit, +s_q, -s_q) ;  idx_q = sum_j bit_q[j] 2^(d-1-j)
        training:  C_q [2^d, d] = +-s_q by the bits of c ;  p = softmax_c(2 tau <r_q, C_q[c]>) ;  H(t) = -sum_c t_c log(clamp(t_c, min=eps))
                   loss_q = w_e (mean_m H(p_m) - gamma H(mean_m p_m)) + w_c mse(r_q, quant_q.detach())      (the mse only when w_c > 0)
        zsum += r_q + (quant_q - r_q).detach() ;  r_{q+1} = r_q - quant_q.detach()
    out = project_out(zsum)  (nn.Linear(d, dim_g) or identity) ; indices of dropped layers (q > k) are -1, their losses 0
  decode: bits of idx_q -> +-s_q, summed over the given columns (-1 contributes zero) ; project_out
  dropout index (host): tests/rvq_train_restated.py's dropout_index, one seed per call shared by all groups
"""
from __future__ import annotations

import math

import torch

from rvq_train_restated import dropout_index  # noqa: F401  (the same host rule as the VQ)

INV_TEMPERATURE = 100.
EPS = 1e-5


def bit_mask(d):
    """int64 [d] = 2^(d-1) .. 1: most significant bit first (the package's per-layer `mask` buffer)"""
    return 2 ** torch.arange(d - 1, -1, -1, dtype=torch.int64)


def codebook(d, scale, dtype=torch.float64):
    """[2^d, d]: row c holds +-scale by the bits of c"""
    bits = (torch.arange(2 ** d, dtype=torch.int64)[:, None] & bit_mask(d)) != 0
    return (bits.to(dtype) * 2 - 1) * scale


def codes_to_indices(r):
    """r [..., d] -> int64 [...]: the index of its sign pattern"""
    return ((r > 0).to(torch.int64) * bit_mask(r.shape[-1])).sum(dim=-1)


def indices_to_codes(idx, d, scale, dtype=torch.float64):
    """int64 [...] -> [..., d] of +-scale (the inverse of codes_to_indices on sign patterns)"""
    bits = (idx.unsqueeze(-1) & bit_mask(d)) != 0
    return (bits.to(dtype) * 2 - 1) * scale


def entropy(t):
    return (-t * torch.log(t.clamp(min=EPS))).sum(dim=-1)


def dense_probs(r, d, scale, inv_temperature=INV_TEMPERATURE):
    """r [M, d] -> softmax over all 2^d codes of -inv_temperature * (-2 <r, C[c]>), as the package writes it"""
    distance = -2 * torch.einsum('md,cd->mc', r, codebook(d, scale, r.dtype))
    return (-distance * inv_temperature).softmax(dim=-1)


def layer(r, q, cfg, train):
    """one LFQ layer on the residual r [M, d] -> (quant with the straight-through graph, hard quant (no graph), idx [M], aux loss scalar)"""
    inv_temperature, w_e, w_c, gamma = cfg
    d, s = r.shape[-1], 2. ** -q
    hard = torch.where(r > 0, torch.full_like(r, s), torch.full_like(r, -s)).detach()
    idx = codes_to_indices(r.detach())
    loss = r.new_zeros(())
    if train:
        p = dense_probs(r, d, s, inv_temperature)
        loss = w_e * (entropy(p).mean() - gamma * entropy(p.mean(dim=0)))
        if w_c > 0:
            loss = loss + w_c * torch.nn.functional.mse_loss(r, hard)
    return r + (hard - r).detach(), hard, idx, loss


def residual_chain(z, Q, k, cfg, train=True):
    """z [M, d] -> (zsum [M, d] with the straight-through graph, idx int64 [M, Q] (-1 past k), losses [Q] (0 past k; zeros without train),
    the residuals r_q [k + 1, M, d] detached)"""
    r, zsum, inds, losses, rs = z, torch.zeros_like(z), [], [], []
    for q in range(Q):
        if q > k:
            inds.append(torch.full(z.shape[:-1], -1, dtype=torch.int64))
            losses.append(z.new_zeros(()))
            continue
        rs.append(r.detach())
        quant, hard, idx, loss = layer(r, q, cfg, train)
        inds.append(idx)
        losses.append(loss)
        zsum = zsum + quant
        r = r - hard
    return zsum, torch.stack(inds, dim=-1), torch.stack(losses), torch.stack(rs)


class GroupLFQ:
    """one group: weights = (W_in [d, dim_g], b_in [d], W_out [dim_g, d], b_out [dim_g]) in the oracle's dtype, or None when dim_g == d;
    cfg = (inv_temperature, entropy_loss_weight, commitment_loss_weight, diversity_gamma)"""

    def __init__(self, codebook_size, num_quantizers, weights=None, cfg=(INV_TEMPERATURE, 0.1, 0., 1.), dtype=torch.float64):
        d = int(codebook_size).bit_length() - 1
        assert codebook_size >= 2 and 2 ** d == codebook_size
        self.d, self.Q, self.dtype, self.cfg = d, num_quantizers, dtype, tuple(float(v) for v in cfg)
        self.weights = weights

    def project_in(self, x):
        return x if self.weights is None else x @ self.weights[0].T + self.weights[1]

    def project_out(self, zsum):
        return zsum if self.weights is None else zsum @ self.weights[2].T + self.weights[3]

    def forward(self, x, k=None, train=True):
        """x [M, dim_g] -> (out [M, dim_g], idx [M, Q], losses [Q], z [M, d], zsum [M, d], r [k + 1, M, d])"""
        k = self.Q - 1 if k is None else k
        z = self.project_in(x)
        zsum, idx, losses, rs = residual_chain(z, self.Q, k, self.cfg, train)
        return self.project_out(zsum), idx, losses, z, zsum, rs

    def decode(self, idx):
        """idx int64 [M, q <= Q] (-1 = no code) -> out [M, dim_g]"""
        zsum = 0.
        for q in range(idx.shape[-1]):
            col = idx[..., q]
            codes = indices_to_codes(col.clamp(min=0), self.d, 2. ** -q, self.dtype)
            zsum = zsum + torch.where((col >= 0).unsqueeze(-1), codes, torch.zeros_like(codes))
        return self.project_out(zsum)


class GroupedLFQ:
    """the grouped form: the last axis split into `groups` chunks, outputs concatenated, indices stacked to (g, b, n, q), losses to (g, q)"""

    def __init__(self, codebook_size, num_quantizers, group_weights, cfg=(INV_TEMPERATURE, 0.1, 0., 1.), dtype=torch.float64):
        self.groups = [GroupLFQ(codebook_size, num_quantizers, w, cfg, dtype) for w in group_weights]

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
        cfg = (rq.inv_temperature, rq.entropy_loss_weight, rq.commitment_loss_weight, rq.diversity_gamma)
        return cls(rq.codebook_size, rq.num_quantizers, ws, cfg, dtype)

    def forward(self, x, k=None, train=True):
        """x (b, n, dim) -> (out (b, n, dim), indices (g, b, n, Q), losses (g, Q), per group r [k + 1, b n, d])"""
        b, n, _ = x.shape
        outs = [grp.forward(ch.reshape(b * n, -1), k, train) for grp, ch in zip(self.groups, x.chunk(len(self.groups), dim=-1))]
        return (torch.cat([o[0].reshape(b, n, -1) for o in outs], dim=-1), torch.stack([o[1].reshape(b, n, -1) for o in outs]),
                torch.stack([o[2] for o in outs]), [o[5] for o in outs])

    def decode(self, indices):
        g, b, n, q = indices.shape
        return torch.cat([grp.decode(indices[i].reshape(b * n, q)).reshape(b, n, -1) for i, grp in enumerate(self.groups)], dim=-1)


# ---------------------------------------------------------------------------------------------- the closed forms the kernels implement

def factorised_log_probs(r, scale, inv_temperature=INV_TEMPERATURE):
    """r [M, d] -> (log P(+) [M, d], log P(-) [M, d]): with a_j = 2 tau s r_j the logit of code c is sum_j sigma_cj a_j, so the softmax over the 2^d
    codes is a product of d two-way softmaxes; log sum_c exp(logit_c) = sum_j (|a_j| + log1p(exp(-2 |a_j|))): no max pass, no overflow"""
    a = 2 * inv_temperature * scale * r
    base = -a.abs() - torch.log1p(torch.exp(-2 * a.abs()))
    return a + base, base - a


def factorised_probs(r, scale, inv_temperature=INV_TEMPERATURE):
    """r [M, d] -> (p [M, 2^d], log p [M, 2^d]) from the per-bit log-probabilities"""
    d = r.shape[-1]
    lp, lm = factorised_log_probs(r, scale, inv_temperature)
    bits = (torch.arange(2 ** d, dtype=torch.int64)[:, None] & bit_mask(d)) != 0                  # [2^d, d]
    logp = torch.where(bits[None], lp[:, None, :], lm[:, None, :]).sum(dim=-1)
    return logp.exp(), logp


def factorised_lse(r, scale, inv_temperature=INV_TEMPERATURE):
    a = (2 * inv_temperature * scale * r).abs()
    return (a + torch.log1p(torch.exp(-2 * a))).sum(dim=-1)


def _fprime(t):
    return -(torch.log(t.clamp(min=EPS)) + (t >= EPS).to(t.dtype))


def closed_form_layer(r, q, cfg):
    """r = r_q [M, d] -> (loss_q, d loss_q / d r_q [M, d]) by the formulas of csrc/lfq.hip"""
    inv_temperature, w_e, w_c, gamma = cfg
    M, d = r.shape
    s = 2. ** -q
    p, logp = factorised_probs(r, s, inv_temperature)
    big = p >= EPS
    h_rows = -(p * torch.where(big, logp, torch.full_like(logp, math.log(EPS)))).sum(dim=-1)
    avg = p.mean(dim=0)
    err = r - torch.where(r > 0, torch.full_like(r, s), torch.full_like(r, -s))
    loss = w_e * (h_rows.mean() - gamma * entropy(avg))
    u = (w_e / M) * (_fprime(p) - gamma * _fprime(avg)[None])
    dlogit = p * (u - (p * u).sum(dim=-1, keepdim=True))
    sigma = codebook(d, 1., r.dtype)                                                              # [2^d, d] of +-1
    grad = 2 * inv_temperature * s * dlogit @ sigma
    if w_c > 0:
        loss = loss + w_c * (err ** 2).mean()
        grad = grad + w_c * 2 * err / (M * d)
    return loss, grad


def closed_form(x, weights, Q, k, cfg, g_out, g_loss):
    """(out, losses [Q], dx, (dW_in, db_in, dW_out, db_out) or ()) of one group by the closed forms: dz = (k + 1) g_z + sum_q g_loss[q] dloss_q/dr_q"""
    z = x if weights is None else x @ weights[0].T + weights[1]
    r, zsum, losses = z, torch.zeros_like(z), []
    g_z = g_out if weights is None else g_out @ weights[2]
    dz = (k + 1) * g_z
    for q in range(Q):
        if q > k:
            losses.append(z.new_zeros(()))
            continue
        loss, grad = closed_form_layer(r, q, cfg)
        losses.append(loss)
        dz = dz + g_loss[q] * grad
        hard = torch.where(r > 0, torch.full_like(r, 2. ** -q), torch.full_like(r, -(2. ** -q)))
        zsum, r = zsum + hard, r - hard
    if weights is None:
        return zsum, torch.stack(losses), dz, ()
    out = zsum @ weights[2].T + weights[3]
    return out, torch.stack(losses), dz @ weights[0], (dz.T @ x, dz.sum(dim=0), g_out.T @ zsum, g_out.sum(dim=0))
