"""The causal flash-attention kernels (csrc/attention.hip: mqa_fwd_kernel, attn_delta_kernel, mqa_bwd_dq_kernel, mqa_bwd_dkv_kernel and their bias / dropout /
QB / NH instantiations) and alm_kv_grad_pack on a real MI355X, through the C ABI, against the float64 restatement tests/attn_restated.py.

Harness.  Every operand with a leading dimension gets a padded one (ldq = H 64 + 8, k | v once interleaved at 128 and once separate at 72, ldo = H 64 + 4,
lddo = H 64 + 8, lddq = H 64 + 4, lddk = 136, part_stride = B N 136 + 24).  Inputs live in arenas (`arena_rows`): the view's last row ends where the data
ends, every pad column and the 64 rows behind the view are NaN -- so a tile DMA whose descriptor ran past row N - 1, or a load of a pad column, poisons a
result.  (One allocation holds view and guard, so the guard is adjacent by construction; two separate allocations need not be.  What it guards is the end of the
LAST batch row's descriptor; in the interleaved layout k's last row is followed by v's data, so the end of the K descriptor is guarded in the separate
layout and in the B = 1 cases.)  Outputs are pre-filled with NaN and followed by guard rows: afterwards pads and guards are still NaN and every valid element is a number.  Every
launch runs twice and the two results are equal bit for bit -- dtbl included: the toeplitz / coarse windows of a (32 query x 64 key) pass span 95 slots,
far inside the dQ kernel's 958-slot LDS window, so its global-atomic fallback (the one documented source of run-to-run differences) is never taken here.

Element-wise bounds: R.bounds -- constants derived in tests/test_attn_host.py from the kernels' bf16 rounding points, times each element's sum of
absolute terms; a dead row / masked key has bound 0 and must be exact.  The backward runs IN ISOLATION: it is fed the restated o rounded to bf16 and the
restated lse in fp32, never the forward kernel's.  dK / dV partials go through alm_kv_grad_pack, and are summed in float64 for the element-wise check.
Shapes and what each input family executes: R.RANDOM, R.RAMPS, R.NEEDLES, R.PREFIX and DESIGN.md 'Causal flash attention: kernel-level tests'."""
import os
import subprocess
import sys

import pytest
import torch

import attn_restated as R

pytestmark = pytest.mark.gpu

BF16, F32, F64, U8, I32 = torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int32
NAN = float('nan')
D = R.DH
LDDK = 136
FORWARD = [n for n in R.case_names() if not n.startswith('needle')]                 # random (every N, H, B of R.RANDOM), the three ramps, the masked prefixes
NEEDLE = [n for n in R.case_names() if n.startswith('needle')]                      # every N, with and without a key mask


@pytest.fixture(scope='module')
def lib():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import _lib, ops
    return type('Lib', (), dict(call=staticmethod(_lib.call), query=staticmethod(_lib.query), ops=ops, st=staticmethod(ops._st)))


def dev():
    return torch.device('cuda:0')


def nan_buf(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def rows(t):
    """(b h n d) -> [B N, H d]"""
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * d)


def unrows(t, B, N, H):
    return t.detach().double().cpu().view(B, N, H, -1).permute(0, 2, 1, 3)


def arena_rows(t2, ld):
    """float64 [rows, W] -> bf16 device view with row pitch ld whose last row ENDS the data: pad columns and the 64 rows after it are NaN"""
    n, W = t2.shape
    buf = nan_buf(((n - 1) * ld + W + 64 * ld,), BF16)
    view = buf.as_strided((n, W), (ld, 1))
    view.copy_(t2.to(BF16))
    return view


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a if isinstance(a[k], torch.Tensor))


def inputs(c, inter):
    """the device operands of one case; inter: k | v interleaved in one [B N, 128] buffer, else two buffers with ld = 72"""
    B, H, N, _ = c['q'].shape
    k2, v2 = c['k'].reshape(B * N, D), c['v'].reshape(B * N, D)
    if inter:
        kv = arena_rows(torch.cat((k2, v2), 1), 2 * D)
        k, v = kv[:, :D], kv[:, D:]
    else:
        k, v = arena_rows(k2, D + 8), arena_rows(v2, D + 8)
    x = dict(q=arena_rows(rows(c['q']), H * D + 8), k=k, v=v, dout=arena_rows(rows(c['dout']), H * D + 8),
             mask=None if c['mask'] is None else c['mask'].to(U8).contiguous().to(dev()), bias=None)
    if c['tbl'] is not None:
        x['bias'] = [c['tbl'].float().contiguous().to(dev()), c['LT']] + [t.to(dev()) for t in c['index']]
    return x


def mask_ptr(x):
    return None if x['mask'] is None else x['mask'].data_ptr()


def forward(lib, c, x):
    """-> dict(o [B N + 1, H 64 + 4], lse [B H N + 64]) as the kernel left them in NaN-filled buffers"""
    B, H, N, _ = c['q'].shape
    W = H * D
    o, lse = nan_buf((B * N + 1, W + 4), BF16), nan_buf((B * H * N + 64,), F32)
    head = [x['q'].data_ptr(), x['q'].stride(0), x['k'].data_ptr(), x['k'].stride(0), x['v'].data_ptr(), x['v'].stride(0), mask_ptr(x), o.data_ptr(), o.stride(0),
            lse.data_ptr(), B, N, H, D, float(c['scale'])]
    tail = [float(c['p']), R.SEED, None, lib.st()]
    if x['bias'] is not None:
        tbl, LT, *idx = x['bias']
        lib.call('alm_mqa_attn_bias_fwd', *head, tbl.data_ptr(), LT, *[t.data_ptr() for t in idx], *tail)
    else:
        lib.call('alm_mqa_attn_fwd', *head, *tail)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse)


def check_fwd_buffers(f, B, N, H, tag):
    W = H * D
    o, lse = f['o'], f['lse']
    assert bool(torch.isnan(o[B * N]).all()) and bool(torch.isnan(o[:B * N, W:]).all()), ('o: a pad column or the guard row was written', tag)
    assert bool(torch.isfinite(o[:B * N, :W].float()).all()), ('o holds NaN / inf: an element was not written, or a pad / guard was read', tag)
    assert bool(torch.isnan(lse[B * H * N:]).all()) and not bool(torch.isnan(lse[:B * H * N]).any()), ('lse guard written or an entry not written', tag)
    return unrows(o[:B * N, :W], B, N, H), lse[:B * H * N].double().cpu().view(B, H, N)


def backward(lib, c, x, o64, lse64):
    """the three backward kernels on the GIVEN o (rounded to bf16 here) and lse (fp32) -> dq, the dk | dv partial sets, the delta workspace, dtbl"""
    B, H, N, _ = c['q'].shape
    W = H * D
    o = nan_buf((B * N, W + 4), BF16)
    o[:, :W] = rows(o64).to(BF16).to(dev())
    lse = lse64.float().contiguous().to(dev())
    parts = lib.query('alm_mqa_bwd_parts', B, N, H)
    stride = B * N * LDDK + 24
    dq, dkv, delta = nan_buf((B * N + 1, W + 4), BF16), nan_buf((parts * stride + LDDK,), F32), nan_buf((2 * B * H * N + 64,), F32)
    head = [x['q'].data_ptr(), x['q'].stride(0), x['k'].data_ptr(), x['k'].stride(0), x['v'].data_ptr(), x['v'].stride(0), mask_ptr(x), o.data_ptr(), o.stride(0),
            lse.data_ptr(), x['dout'].data_ptr(), x['dout'].stride(0), dq.data_ptr(), dq.stride(0), dkv.data_ptr(), dkv.data_ptr() + 4 * D, LDDK, stride,
            delta.data_ptr(), B, N, H, D, float(c['scale'])]
    tail = [float(c['p']), R.SEED, None, lib.st()]
    out = dict(dq=dq, dkv=dkv, delta=delta, parts=parts, stride=stride)
    if x['bias'] is not None:
        tbl, LT, *idx = x['bias']
        prow = lib.query('alm_attn_bias_part_rows', B, N, H)
        part = torch.zeros((prow + 1, LT), dtype=F32, device=dev())
        part[prow] = NAN
        lib.call('alm_mqa_attn_bias_bwd', *head, tbl.data_ptr(), LT, *[t.data_ptr() for t in idx], part.data_ptr(), *tail)
        dtbl = nan_buf((H + 1, LT), F32)
        lib.call('alm_attn_bias_grad_reduce', part.data_ptr(), dtbl.data_ptr(), B, N, H, LT, float(c['scale']), lib.st())
        out.update(part=part, dtbl=dtbl)
    else:
        lib.call('alm_mqa_attn_bwd', *head, *tail)
    # the product's own sum of the partial sets: alm_kv_grad_pack (mode 0), into a padded NaN buffer
    packed = nan_buf((B * N + 1, LDDK), BF16)
    lib.call('alm_kv_grad_pack', dkv.data_ptr(), dkv.data_ptr() + 4 * D, LDDK, parts, stride, None, packed.data_ptr(), LDDK, B * N, D, 0, lib.st())
    torch.cuda.synchronize()
    out['packed'] = packed
    return out


def check_bwd_buffers(r, B, N, H, tag):
    """pads / guards still NaN, valid elements numbers -> (dq, dk, dv, ndelta, nlse[, dtbl]) in float64 on the host; dk / dv: the float64 sum of the sets"""
    W, parts, stride = H * D, r['parts'], r['stride']
    dq = r['dq']
    assert bool(torch.isnan(dq[B * N]).all()) and bool(torch.isnan(dq[:B * N, W:]).all()), ('dq: a pad column or the guard row was written', tag)
    assert bool(torch.isfinite(dq[:B * N, :W].float()).all()), ('dq holds NaN / inf', tag)
    sets = r['dkv'][:parts * stride].view(parts, stride)
    valid = sets[:, :B * N * LDDK].view(parts, B * N, LDDK)
    assert bool(torch.isnan(r['dkv'][parts * stride:]).all()) and bool(torch.isnan(sets[:, B * N * LDDK:]).all()) and bool(torch.isnan(valid[..., 2 * D:]).all()), \
        ('dk / dv: written between the partial sets, past the last one or in a pad column', tag)
    assert bool(torch.isfinite(valid[..., :2 * D]).all()), ('dk / dv partials hold NaN / inf', tag)
    n = B * H * N
    assert bool(torch.isnan(r['delta'][2 * n:]).all()) and bool(torch.isfinite(r['delta'][:n]).all()) and not bool(torch.isnan(r['delta'][n:2 * n]).any()), ('delta workspace', tag)
    total = valid[..., :2 * D].double().sum(0).cpu()
    pk = r['packed']
    assert bool(torch.isnan(pk[B * N]).all()) and bool(torch.isnan(pk[:B * N, 2 * D:]).all()), ('alm_kv_grad_pack wrote a pad column or the guard row', tag)
    terms = valid[..., :2 * D].double().abs().sum(0).cpu()
    e_pack = R.ratio(pk[:B * N, :2 * D].double().cpu(), total, 2 * (R.U * total.abs() + 2.0 ** -20 * terms))
    assert e_pack <= 1., ('alm_kv_grad_pack: not the sum of the partial sets rounded once', tag, e_pack)
    out = dict(dq=unrows(dq[:B * N, :W], B, N, H), dk=total[:, :D].view(B, N, D), dv=total[:, D:].view(B, N, D),
               ndelta=r['delta'][:n].double().cpu().view(B, H, N), nlse=r['delta'][n:2 * n].double().cpu().view(B, H, N), pack=e_pack)
    if 'dtbl' in r:
        assert bool(torch.isnan(r['dtbl'][H]).all()) and bool(torch.isnan(r['part'][-1]).all()) and bool(torch.isfinite(r['dtbl'][:H]).all()), ('dtbl', tag)
        out['dtbl'] = r['dtbl'][:H].double().cpu()
    return out


def check_forward(lib, name, inter):
    """forward twice, buffers, o and lse element-wise -> worst error / bound"""
    c = R.case(name)
    ref, _, bound = R.reference(name)
    B, H, N, _ = c['q'].shape
    x = inputs(c, inter)
    f = forward(lib, c, x)
    assert same_bits(f, forward(lib, c, x)), ('two forward launches differ', name)
    o, lse = check_fwd_buffers(f, B, N, H, name)
    dead = torch.isinf(ref['lse'])
    assert torch.equal(torch.isinf(lse), dead) and bool((lse[dead] == float('-inf')).all()), ('lse -inf pattern', name)
    assert float(o[dead[..., None].expand_as(o)].abs().sum()) == 0., ('a dead row of o is not exactly 0', name)
    r_o = R.ratio(o, ref['o'], bound['o'])
    r_l = R.ratio(lse[~dead], ref['lse'][~dead], bound['lse'][~dead])
    return r_o, r_l, x, o, lse


def check_backward(lib, name, x=None, inter=True):
    """backward in isolation, twice, buffers, every output element-wise -> dict of worst error / bound"""
    c = R.case(name)
    ref, T, bound = R.reference(name)
    B, H, N, _ = c['q'].shape
    x = x or inputs(c, inter)
    r = backward(lib, c, x, ref['o'], ref['lse'])
    assert same_bits(r, backward(lib, c, x, ref['o'], ref['lse'])), ('two backward launches differ', name)
    g = check_bwd_buffers(r, B, N, H, name)
    o_b, lse32 = R.bf(ref['o']), ref['lse'].float().double()
    nd, nl = R.delta(o_b, c['dout'], lse32, c['scale'])
    dead = torch.isinf(ref['lse'])
    assert torch.equal(torch.isinf(g['nlse']), dead) and bool((g['nlse'][dead] == float('-inf')).all()), ('nlse -inf pattern', name)
    # ndelta: products of two bf16 numbers are exact in fp32; 7 additions per lane + 3 across lanes, each u32 of the absolute terms: 16 u32 bounds them.
    # nlse = -lse (1 / scale): one fp32 rounding (none at all for scale = 1/8)
    rs = dict(ndelta=R.ratio(g['ndelta'], nd, 16 * 2.0 ** -24 * (c['dout'] * o_b).abs().sum(-1) + 1e-30),
              nlse=R.ratio(g['nlse'][~dead], nl[~dead], 2.0 ** -24 * nl[~dead].abs() + 1e-30), pack=g['pack'])
    assert float(g['dq'][dead[..., None].expand_as(g['dq'])].abs().sum()) == 0., ('dq of a dead row is not exactly 0', name)
    if c['mask'] is not None:
        assert float(g['dk'][~c['mask']].abs().sum()) == 0. and float(g['dv'][~c['mask']].abs().sum()) == 0., ('a masked key received a gradient', name)
    for n in ('dq', 'dk', 'dv') + (('dtbl',) if 'dtbl' in g else ()):
        rs[n] = R.ratio(g[n], ref[n], bound[n])
    return rs, g


def report(name, rs):
    print(f'{name}: error / bound  ' + '  '.join(f'{k} {v:.3f}' for k, v in rs.items()))
    bad = {k: v for k, v in rs.items() if not v <= 1.}
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize('name', FORWARD)
def test_forward_elementwise(lib, name):
    """o and lse against the float64 restatement on the random inputs (every N of R.NS once: one 32-query block, the diagonal at every offset, N = 96: the
    npass == 1 middle block; H = 1, 3, 5: inactive waves, H = 5, 8: a second head group; rand-4x129x8: decode_block's XCD branches with an odd block
    count), the three ramps (raise every tile / m stale over tiles with P up to 2^7 / first tile holds the maximum) and the masked prefixes (dead rows,
    key tiles masked while m = -inf).  k | v interleaved for every other case, separate buffers with ld = 72 for the rest"""
    r_o, r_l, *_ = check_forward(lib, name, FORWARD.index(name) % 2 == 0)
    report(name, dict(o=r_o, lse=r_l))


@pytest.mark.parametrize('name', NEEDLE)
def test_forward_needles(lib, name):
    """every query's whole answer is ONE key (64 nats, >= 30 above the next): o must equal v[target] bit for bit and lse 64 -- a key lost or doubled at any
    (query lane, key lane, tile) position changes some row completely, which no norm over the tensor can hide"""
    c = R.case(name)
    B, H, N, _ = c['q'].shape
    r_o, r_l, x, o, lse = check_forward(lib, name, NEEDLE.index(name) % 4 < 2)
    live = c['target'] >= 0
    want = torch.gather(c['v'][:, None].expand(B, H, N, D), 2, c['target'].clamp(min=0)[..., None].expand(B, H, N, D))
    wrong = ((o != want).any(-1) & live).nonzero()
    assert len(wrong) == 0, (name, 'o != v[target] at (b, h, query)', wrong[:8].tolist(), 'targets', c['target'][tuple(wrong[:8].t())].tolist())
    e = float((lse[live] - 64.).abs().max()) if bool(live.any()) else 0.
    print(f'{name}: o == v[target] bit for bit on {int(live.sum())} queries, |lse - 64| <= {e:.1e}')
    assert e <= 1e-4, (name, e)


# ------------------------------------------------------------------------------------------------ backward, in isolation

@pytest.mark.parametrize('name', FORWARD)
def test_backward_in_isolation(lib, name):
    """dq, dk, dv (float64 sum of the partial sets; the sets also go through alm_kv_grad_pack), ndelta and nlse element-wise, fed the RESTATED o (bf16) and
    lse (fp32).  The ramps put P near 1 at the diagonal and run exp2(S c2 - lse2) over +-28 nats; the prefixes: dead rows (dq exactly 0) and masked keys
    (dk, dv exactly 0)"""
    rs, _ = check_backward(lib, name, inter=FORWARD.index(name) % 2 == 1)
    report(name, rs)


@pytest.mark.parametrize('name', NEEDLE)
def test_backward_needles(lib, name):
    """P is the one-hot of the target: dv[j] is the sum of the dO rows of the queries that target j (fp32 summation error only), dq and dk are 0 within
    their bounds (dP - delta cancels to fp32 noise)"""
    c = R.case(name)
    ref, T, _ = R.reference(name)
    rs, g = check_backward(lib, name, inter=NEEDLE.index(name) % 4 >= 2)
    B, H, N, _ = c['q'].shape
    want, mag = torch.zeros(B, N, D, dtype=F64), torch.zeros(B, N, D, dtype=F64)
    live = c['target'] >= 0
    for b in range(B):
        want[b].index_add_(0, c['target'][b][live[b]], c['dout'][b][live[b]])
        mag[b].index_add_(0, c['target'][b][live[b]], c['dout'][b][live[b]].abs())
    # (the other keys hold <= 1e-9 of a query's mass, asserted on the host: at most that share of every dO row reaches a key that is nobody's target)
    rs['dv_rows'] = R.ratio(g['dv'], want, 2.0 ** -16 * mag + 1e-9 * c['dout'].abs().sum((1, 2))[:, None, :])
    report(name, rs)


# ------------------------------------------------------------------------------------------------ masked K / V rows are never used

@pytest.mark.parametrize('name', ['prefix', 'rand-2x200x5-m', 'rand-4x129x8-m'])
def test_masked_kv_rows_do_not_reach_any_output(lib, name):
    """the K and V rows of key-masked positions go from 0 to +-2^10: every output of the forward and of the backward is unchanged bit for bit (the dK/dV
    kernel lets such a key's COLUMN hold anything off the diagonal and selects zero for it in the epilogue)"""
    c = R.case(name)
    ref, _, _ = R.reference(name)
    hid = ~c['mask'][..., None]
    g = R.gen(3)
    big = (torch.randint(0, 2, c['k'].shape, generator=g) * 2 - 1).double() * 1024.
    outs = []
    for fill in (torch.zeros(()).double(), big):
        cc = dict(c, k=torch.where(hid, fill, c['k']), v=torch.where(hid, fill, c['v']))
        x = inputs(cc, True)
        outs.append(dict(forward(lib, cc, x), **{k: v for k, v in backward(lib, cc, x, ref['o'], ref['lse']).items()}))
    assert same_bits(outs[0], outs[1]), name
    B, H, N, _ = c['q'].shape
    check_fwd_buffers(outs[1], B, N, H, name), check_bwd_buffers(outs[1], B, N, H, name)


# ------------------------------------------------------------------------------------------------ bias and dropout instantiations

@pytest.mark.parametrize('name', R.variant_names())
def test_bias_and_dropout_instantiations(lib, name):
    """{no bias, toeplitz, coarse (special pairs: slot 0)} x {p = 0, 0.25} on the masked prefixes (dead rows in every instantiation) and the raising ramp:
    alm_mqa_attn_bias_fwd / _bwd + alm_attn_bias_grad_reduce and the DROP kernels with the restated keep mask; the same element-wise bounds, and dtbl
    against the restated table gradient"""
    from audiolm_pytorch_amd import relpos
    c = R.case(name)
    if c['index'] is not None:
        N = c['q'].shape[2]
        mine = relpos.toeplitz_index(N, dev(), num_leading=N // 3 + 1 if '+coarse+' in name else None)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(mine, c['index']))
    r_o, r_l, x, *_ = check_forward(lib, name, True)
    rs, _ = check_backward(lib, name, x=x)
    report(name, dict(o=r_o, lse=r_l, **rs))


# ------------------------------------------------------------------------------------------------ alm_kv_grad_pack

@pytest.mark.parametrize('nparts', [1, 2, 4])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_kv_grad_pack(lib, nparts, mode):
    """1, 2 and 4 partial sets, the three value-residual modes, ld = 136, part_stride = rows 136 + 24, ldo = 136: the float64 sum rounded once"""
    rows_ = 77
    g = R.gen(5 + nparts)
    parts, acc = torch.randn(nparts, rows_, 2 * D, generator=g).float(), torch.randn(rows_, D, generator=g).float()
    stride = rows_ * LDDK + 24
    buf = nan_buf((nparts * stride + LDDK,), F32)
    buf[:nparts * stride].view(nparts, stride)[:, :rows_ * LDDK].view(nparts, rows_, LDDK)[..., :2 * D] = parts.to(dev())
    outs = []
    for _ in range(2):
        a = torch.cat((acc.to(dev()).flatten(), nan_buf((64,), F32)))
        out = nan_buf((rows_ + 1, LDDK), BF16)
        lib.call('alm_kv_grad_pack', buf.data_ptr(), buf.data_ptr() + 4 * D, LDDK, nparts, stride, a.data_ptr() if mode else None, out.data_ptr(), LDDK, rows_, D,
                 mode, lib.st())
        torch.cuda.synchronize()
        outs.append(dict(out=out, a=a))
    assert same_bits(outs[0], outs[1])
    out, a = outs[0]['out'], outs[0]['a']
    assert bool(torch.isnan(out[rows_]).all()) and bool(torch.isnan(out[:rows_, 2 * D:]).all()) and bool(torch.isnan(a[rows_ * D:]).all())
    want, acc2 = R.kv_grad_pack(parts.double(), acc.double(), mode)
    terms, tacc = R.kv_grad_pack(parts.double().abs(), acc.double().abs(), mode)
    rs = dict(dkv=R.ratio(out[:rows_, :2 * D].double().cpu(), want, 2 * (R.U * want.abs() + 2.0 ** -20 * terms)),
              acc=R.ratio(a[:rows_ * D].double().cpu().view(rows_, D), acc2, 2.0 ** -20 * tacc))
    report(f'kv_grad_pack nparts={nparts} mode={mode}', rs)


# ------------------------------------------------------------------------------------------------ policy hooks

def test_backward_partial_sets_follow_the_policy_in_force(lib):
    """alm_mqa_bwd_parts under whatever ALM_ATTN_DKV_NH / ALM_ATTN_DKV_SPLIT this interpreter was started with: (heads per workgroup: forced, else 4 below
    N = 8192) x (SPLIT-Q: forced, else 2 while N > 64 and the doubled launch stays within 256 workgroups).  Selected by the forced-policy runs below, so a
    child in which the variable did not arrive fails here"""
    nh_env, sp_env = os.environ.get('ALM_ATTN_DKV_NH'), os.environ.get('ALM_ATTN_DKV_SPLIT')
    for B, N, H in [(1, 5, 3), (2, 64, 8), (1, 129, 3), (3, 129, 5), (4, 129, 8), (2, 200, 5), (8, 641, 8), (1, 8253, 8)]:
        nh = int(nh_env) if nh_env in ('2', '4') else (2 if N >= 8192 else 4)
        groups = (H + nh - 1) // nh
        split = int(sp_env) if sp_env in ('1', '2') else (2 if N > 64 and 2 * ((N + 63) // 64) * groups * B <= 256 else 1)
        assert lib.query('alm_mqa_bwd_parts', B, N, H) == groups * split, (B, N, H, nh_env, sp_env)

@pytest.mark.parametrize('env', ['ALM_ATTN_FWD_QB2_MINN=1', 'ALM_ATTN_DKV_SPLIT=1', 'ALM_ATTN_DKV_SPLIT=2', 'ALM_ATTN_DKV_NH=2'])
def test_the_forced_policies_pass_the_same_tests(env):
    """the QB = 2 forward, the dK/dV kernel without / with SPLIT-Q at every N (the automatic policy splits only for N > 64 and at most 128 workgroups) and
    with 2 heads per workgroup: each is a process-wide policy read once, so each forced value runs this file's unbiased, no-dropout tests in its own
    interpreter, one at a time.  ALM_ATTN_DKV_NH / _SPLIT are seen to arrive through alm_mqa_bwd_parts (test_backward_partial_sets_follow_the_policy_in_force);
    ALM_ATTN_FWD_QB2_MINN has no observable in the C ABI: that the child took the QB = 2 kernel is ASSUMED from the variable being in its environment"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, v = env.split('=')
    r = subprocess.run([sys.executable, '-m', 'pytest', 'tests/test_gpu_attn_kernels.py', '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider',
                        '-k', 'forward_ or backward_ or masked_kv'], cwd=root, env=dict(os.environ, **{k: v}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout
