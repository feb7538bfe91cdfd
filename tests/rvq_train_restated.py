"""TEST INFRASTRUCTURE ONLY.  Plain-torch restatement of the TRAINING-mode forward of vector-quantize-pytorch's `GroupedResidualVQ` as the reference
builds it (audiolm_pytorch/soundstream.py:592-607: decay = rq_ema_decay, commitment_weight, kmeans_init with 10 iterations, threshold_ema_dead_code = 2,
quantize_dropout with cutoff index and multiple_of, rotation_trick, eps = 1e-5; stochastic_sample_codes unsupported).  Runs on the CPU in float64 or
float32; gradients come from torch autograd of this forward, never from hand-written formulas.  The eval-mode forward is oracle/rvq_restated.py's,
operation for operation.

PARITY UNPINNED: the upstream library is not vendored and no golden vectors of it exist here.  The arithmetic below is this project's specification of
the training step; where a detail of the upstream library differs, this text wins:

  per group (features chunked along the last dim), M = b * n rows:
    residual = x_g ; out = 0 ; k = dropout index ; layers q > k: indices -1, loss 0, no state change
    for q in 0..k:
        if not initted[q]: k-means init on `residual`
        idx   = argmin_c sqrt(clamp(|r|^2 + |e_c|^2 - 2 r.e_c, 0)), first index on ties (the PRE-update embed)
        quant = embed[idx]
        loss_q = commitment_weight * mean over all M * d elements of (quant.detach() - residual)^2
        rotation trick: u = r / |r|, qh = quant / |quant| (0 where the norm is 0), w = normalize(u + qh) (eps 1e-12), lam = |quant| / |r| (0 where |r| = 0),
                        all DETACHED:  y = lam * (r - 2 (r.w) w + 2 (r.u) qh);      otherwise  y = r + (quant - r).detach()
        residual = residual - y.detach() ; out = out + y
    after the layer loop, for q in 0..k (neither step influences a later layer of the same call, so the order is free; the sampled rows are drawn in
    this order), on the statistics of this call's assignments and layer q's INPUT residual:
        n_c = #rows with idx == c ; s_c = their sum
        cluster_size = cluster_size * decay + n * (1 - decay) ; embed_avg = embed_avg * decay + s * (1 - decay)
        smoothed = (cluster_size + eps) / (sum(cluster_size) + C eps) * sum(cluster_size) ; embed = embed_avg / smoothed[:, None]
        expiry: codes with cluster_size < threshold (ascending) get embed = a sampled row of the residual, cluster_size = threshold,
                embed_avg = threshold * that row
  dropout index (host): seed = random.randint(0, 1e7) once per call, k = random.Random(seed).randrange(cutoff, Q); multiple_of m != 1: k = ceil((k + 1) / m) m - 1
  sampled rows, `count` of M: torch.randperm(M)[:count] when M >= count, else torch.randint(0, M, (count,))
  k-means init: means = sampled rows; 10 x (assign with the distance above, bins = per-code counts, means = where(bins == 0, means, sums / max(bins, 1)));
                embed = means, cluster_size = the last bins, embed_avg = means * bins[:, None], initted = True
"""
from __future__ import annotations

import random

import torch
import torch.nn.functional as F


def default_sample_rows(num_rows, count):
    if num_rows >= count:
        return torch.randperm(num_rows)[:count]
    return torch.randint(0, num_rows, (count,))


def dropout_index(num_quantizers, cutoff, multiple_of, quantize_dropout=True):
    if not quantize_dropout or num_quantizers <= 1:
        return num_quantizers - 1
    seed = random.randint(0, int(1e7))
    k = random.Random(seed).randrange(cutoff, num_quantizers)
    if multiple_of != 1:
        k = -(-(k + 1) // multiple_of) * multiple_of - 1
    return min(k, num_quantizers - 1)


def distances(flat, embed):
    """-sqrt(clamp(|x|^2 + |e|^2 - 2 x.e, 0)) as oracle/rvq_restated.py forms it: flat (1, M, d), embed (1, C, d) -> (1, M, C)"""
    x2 = (flat ** 2).sum(dim=-1)
    y2 = (embed ** 2).sum(dim=-1)
    xy = torch.einsum('bid,bjd->bij', flat, embed) * -2
    return -(x2.unsqueeze(-1) + y2.unsqueeze(-2) + xy).clamp(min=0).sqrt()


def _safe_div(a, b):
    ok = b != 0
    return torch.where(ok, a / torch.where(ok, b, torch.ones_like(b)), torch.zeros_like(a))


def rotate_to(r, quant):
    rd, qd = r.detach(), quant.detach()
    rn, qn = rd.norm(dim=-1, keepdim=True), qd.norm(dim=-1, keepdim=True)
    u, qh = _safe_div(rd, rn), _safe_div(qd, qn)
    w = F.normalize(u + qh, dim=-1)
    lam = _safe_div(qn, rn)
    return lam * (r - 2 * (r * w).sum(-1, keepdim=True) * w + 2 * (r * u).sum(-1, keepdim=True) * qh)


class TrainRVQ:
    """state[g][q] = dict(initted: bool, cluster_size [C], embed_avg [C, d], embed [C, d]) in `dtype` on the CPU"""

    def __init__(self, *, dim, groups=1, num_quantizers, codebook_size, decay=0.95, commitment_weight=1., quantize_dropout=True,
                 quantize_dropout_cutoff_index=1, quantize_dropout_multiple_of=1, rotation_trick=True, threshold_ema_dead_code=2, kmeans_iters=10,
                 eps=1e-5, dtype=torch.float64, sample_rows=default_sample_rows):
        assert dim % groups == 0
        self.dim, self.groups, self.num_quantizers, self.codebook_size = dim, groups, num_quantizers, codebook_size
        self.decay, self.commitment_weight, self.eps = decay, commitment_weight, eps
        self.quantize_dropout, self.cutoff, self.multiple_of = quantize_dropout, quantize_dropout_cutoff_index, quantize_dropout_multiple_of
        self.rotation_trick, self.threshold, self.kmeans_iters = rotation_trick, threshold_ema_dead_code, kmeans_iters
        self.dtype, self.sample_rows = dtype, sample_rows
        d = dim // groups
        self.state = [[dict(initted=False, cluster_size=torch.ones(codebook_size, dtype=dtype), embed_avg=torch.zeros(codebook_size, d, dtype=dtype),
                            embed=torch.zeros(codebook_size, d, dtype=dtype)) for _ in range(num_quantizers)] for _ in range(groups)]
        self.kmeans_empty = 0                 # empty clusters met in k-means rounds so far
        self.min_gap = float('inf')           # smallest (d2 - d1) / d1 over every assignment made so far (incl. the k-means rounds)

    def load_module(self, rq):
        """copies the buffers of a module with the upstream tree (rvqs.{g}.layers.{q}._codebook.*)"""
        for g, r in enumerate(rq.rvqs):
            for q, l in enumerate(r.layers):
                cb, st = l._codebook, self.state[g][q]
                st['initted'] = bool(cb.initted.item())
                st['cluster_size'] = cb.cluster_size.detach()[0].cpu().to(self.dtype).clone()
                st['embed_avg'] = cb.embed_avg.detach()[0].cpu().to(self.dtype).clone()
                st['embed'] = cb.embed.detach()[0].cpu().to(self.dtype).clone()
        return self

    def _assign(self, r, embed):
        dist = distances(r.unsqueeze(0), embed.unsqueeze(0))[0]               # (M, C), negated distances
        self._note_gap(dist)
        return dist.argmax(dim=-1)

    def _note_gap(self, dist):
        if dist.shape[-1] > 1:
            top = (-dist).topk(2, dim=-1, largest=False).values
            gap = _safe_div(top[:, 1] - top[:, 0], top[:, 0])
            gap = torch.where(top[:, 0] == 0, torch.where(top[:, 1] > 0, float('inf'), 0.).to(gap.dtype), gap)       # an exact tie is a gap of 0
            self.min_gap = min(self.min_gap, float(gap.min()))

    def _stats(self, r, idx):
        C = self.codebook_size
        n = torch.zeros(C, dtype=r.dtype).index_add_(0, idx, torch.ones(r.shape[0], dtype=r.dtype))
        s = torch.zeros(C, r.shape[1], dtype=r.dtype).index_add_(0, idx, r)
        return n, s

    def _kmeans(self, r, st):
        means = r[self.sample_rows(r.shape[0], self.codebook_size)].clone()
        bins = None
        for _ in range(self.kmeans_iters):
            bins, s = self._stats(r, self._assign(r, means))
            self.kmeans_empty += int((bins == 0).sum())
            means = torch.where((bins == 0)[:, None], means, s / bins.clamp(min=1)[:, None])
        st['embed'], st['cluster_size'], st['embed_avg'], st['initted'] = means, bins.clone(), means * bins[:, None], True

    def _update(self, st, r, idx):
        n, s = self._stats(r, idx)
        cs = st['cluster_size'] * self.decay + n * (1 - self.decay)
        ea = st['embed_avg'] * self.decay + s * (1 - self.decay)
        tot = cs.sum()
        smoothed = (cs + self.eps) / (tot + self.codebook_size * self.eps) * tot
        embed = ea / smoothed[:, None]
        if self.threshold > 0:
            dead = (cs < self.threshold).nonzero()[:, 0]
            if dead.numel():
                rows = r[self.sample_rows(r.shape[0], dead.numel())]
                embed[dead], cs[dead], ea[dead] = rows, float(self.threshold), rows * float(self.threshold)
        st['cluster_size'], st['embed_avg'], st['embed'] = cs, ea, embed

    def _group_train(self, xg, g, k):
        M, d = xg.shape
        residual, out = xg, torch.zeros_like(xg)
        inds, losses, pending = [], [], []
        for q in range(self.num_quantizers):
            if q > k:
                inds.append(torch.full((M,), -1, dtype=torch.int64)), losses.append(torch.zeros((), dtype=xg.dtype))
                continue
            st, r = self.state[g][q], residual.detach()
            if not st['initted']:
                self._kmeans(r, st)
            idx = self._assign(r, st['embed'])
            quant = st['embed'][idx]
            losses.append(self.commitment_weight * ((quant.detach() - residual) ** 2).mean())
            y = rotate_to(residual, quant) if self.rotation_trick else residual + (quant - residual).detach()
            pending.append((st, r, idx))
            residual, out = residual - y.detach(), out + y
            inds.append(idx)
        for st, r, idx in pending:
            self._update(st, r, idx)
        return out, torch.stack(inds, dim=-1), torch.stack(losses)

    def _group_eval(self, xg, g):
        residual, out, inds = xg, 0., []
        for st in self.state[g]:
            assert st['initted'], 'restated RVQ needs explicitly initialised codebooks'
            embed = st['embed'].unsqueeze(0)
            flat = residual.reshape(1, -1, residual.shape[-1])
            dist = distances(flat, embed)
            self._note_gap(dist[0])
            ind = dist.argmax(dim=-1)
            quant = embed[0][ind[0]].reshape(residual.shape)
            residual, out = residual - quant, out + quant
            inds.append(ind.reshape(residual.shape[:-1]))
        return out, torch.stack(inds, dim=-1), torch.zeros(len(self.state[g]))

    def forward(self, x, training=True, k=None):
        """x (b, n, dim) in self.dtype -> (out (b, n, dim), indices (g, b, n, Q) int64, losses (g, Q)); k: forced dropout index"""
        b, n, _ = x.shape
        chunks = x.chunk(self.groups, dim=-1)
        if training:
            if k is None:
                k = dropout_index(self.num_quantizers, self.cutoff, self.multiple_of, self.quantize_dropout)
            outs = [self._group_train(c.reshape(b * n, -1), g, k) for g, c in enumerate(chunks)]
            outs = [(o.reshape(b, n, -1), i.reshape(b, n, -1), l) for o, i, l in outs]
        else:
            outs = [self._group_eval(c, g) for g, c in enumerate(chunks)]
        return torch.cat([o[0] for o in outs], dim=-1), torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs])


# ---- per-kernel references of csrc/rvq_train.hip (tests/test_gpu_rvq_train_kernels.py).  Indices are INPUTS here (-1 or >= C: the row takes no part);
# each function restates one `ops.rvq_*` call with the arithmetic of TrainRVQ above.  tests/test_rvq_train_host.py composes them into one training
# step and finds TrainRVQ.forward + autograd again, so the GPU tests rest on references that are themselves checked without a GPU.

def _taking_part(idx, C):
    return (idx >= 0) & (idx < C)


def layer_y(r, quant, rotation):
    return rotate_to(r, quant) if rotation else r + (quant - r).detach()


def code_stats_ref(r, idx, C):
    """ops.rvq_code_stats: n [C] rows per code, s [C, d] their sums (TrainRVQ._stats over the rows that take part)"""
    keep = _taking_part(idx, C)
    n = torch.zeros(C, dtype=r.dtype).index_add_(0, idx[keep], torch.ones(int(keep.sum()), dtype=r.dtype))
    s = torch.zeros(C, r.shape[1], dtype=r.dtype).index_add_(0, idx[keep], r[keep])
    return n, s


def quantize_ref(resid, idx, E, out, loss_scale, rotation):
    """ops.rvq_train_quantize of one layer -> (resid - y, out + y, loss_scale * sum |E[idx] - resid|^2, y); rows that take no part keep resid and out"""
    keep = _taking_part(idx, E.shape[0])
    quant = E[idx.clamp(0, E.shape[0] - 1)]
    y = torch.where(keep[:, None], layer_y(resid, quant, rotation), torch.zeros_like(resid))
    loss = loss_scale * (torch.where(keep[:, None], quant.detach() - resid, torch.zeros_like(resid)) ** 2).sum()
    return resid - y.detach(), out + y, loss, y


def layer_residual_ref(x, idx, E, q, rotation):
    """the input residual of layer q of every row of x [M, d], from idx [M, Q] and the codebooks E [Q, C, d] (a layer with no code is a no-op)"""
    resid = x.detach()
    for l in range(q):
        resid = quantize_ref(resid, idx[:, l], E[l], torch.zeros_like(resid), 0., rotation)[0]
    return resid


def bwd_ref(x, idx, E, g_out, coef, rotation):
    """ops.rvq_train_bwd: autograd of sum(out * g_out) + sum_l coef_l / 2 |r_l - E_l[idx_l]|^2 over the chain of quantize_ref (g_out, coef: None = absent)"""
    x = x.detach().clone().requires_grad_()
    resid, out, total = x, torch.zeros_like(x), x.sum() * 0
    for l in range(E.shape[0]):
        resid, out, loss, _ = quantize_ref(resid, idx[:, l], E[l], out, 0.5 if coef is None else 0.5 * coef[l], rotation)
        if coef is not None:
            total = total + loss
    if g_out is not None:
        total = total + (out * g_out).sum()
    total.backward()
    return x.grad


def ema_update_ref(cluster_size, embed_avg, n, s, decay, eps, threshold):
    """ops.rvq_ema_update (TrainRVQ._update before the expiry) -> (cluster_size, embed_avg, embed, the ascending list of the codes below the threshold)"""
    cs = cluster_size * decay + n * (1 - decay)
    ea = embed_avg * decay + s * (1 - decay)
    tot = cs.sum()
    smoothed = (cs + eps) / (tot + cs.numel() * eps) * tot
    dead = (cs < threshold).nonzero()[:, 0] if threshold > 0 else torch.zeros(0, dtype=torch.int64)
    return cs, ea, ea / smoothed[:, None], dead


def expire_ref(codes, rows, x, idx, E, q, rotation, threshold, cluster_size, embed_avg, embed):
    """ops.rvq_expire -> the three buffers after it: each listed (code, row) with 0 <= code < C and 0 <= row < M gets embed = the layer-q residual of
    that row, cluster_size = threshold, embed_avg = threshold * that residual; any other entry is skipped"""
    cs, ea, em = cluster_size.clone(), embed_avg.clone(), embed.clone()
    resid = layer_residual_ref(x, idx, E, q, rotation)
    for code, row in zip(codes.tolist(), rows.tolist()):
        if 0 <= code < em.shape[0] and 0 <= row < x.shape[0]:
            em[code], cs[code], ea[code] = resid[row], float(threshold), resid[row] * float(threshold)
    return cs, ea, em


def kmeans_update_ref(means, n, s):
    """ops.rvq_kmeans_update: an empty bin keeps its mean, the others become s / max(n, 1)"""
    return torch.where((n == 0)[:, None], means, s / n.clamp(min=1)[:, None])
