"""GPU: audiolm_pytorch_amd.T5Encoder (csrc/t5.hip through the C ABI) against the restated T5 encoder (tests/t5_restated.py) in fp64 on the host.

Per-kernel bounds are first-order rounding bounds evaluated in fp64 from the same operands (u = 2^-24); none is taken from what the kernels return:
  norm       sum of C squares in two levels (C / 32 per slice, 32 slices): rstd carries <= (C / 64 + 17) u, the rest of the formula <= 8 u
  gate       the argument of tanh carries 4 u relative, tanh' <= 1 and |arg| (1 - tanh^2) < 0.5: |d(1 + tanh)| <= 8 u -> |d gelu_new| <= 8 u (|a| + |g|)
  attention  a score is a 64-term dot product plus the bias: ds <= 66 u sum |q k| + 2 u |s|; a weight exp(s - m) then carries 2 ds + u |s - m| + 4 u
             relative, the running rescale 3 u per key tile, the two sums T u: |d o| <= (4 ds + 2 u max|s - m| + (T + 4 tiles + 16) u) sum_j p_j |v_j|;
             that worst case is loose, so attention also has to stay within 8 x the error of the same formula in fp32 on the CPU (per query, L2)
The whole-model bound is the one the feature was specified with: max over valid positions of the per-position L2 error, relative to the position's
norm, at most 8 x the same statistic of the restatement run in fp32 on the CPU (r_nat <= 8 r_cpu).

Measured on an MI355X (this file, -s): see DESIGN.md section 'T5 text encoder'.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import t5_restated as TR
from common import GOLDEN_DIR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F64 = torch.float64
NAME = 'local/t5-gpu-test'


def dev():
    return torch.device('cuda:0')


def A():
    import audiolm_pytorch_amd
    return audiolm_pytorch_amd


def OPS():
    from audiolm_pytorch_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def check(got, want, tol, what):
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / tol).max())
    print(f'{what}: max abs err {float(err.max()):.3e}, max err / bound {ratio:.3f}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (what, ratio)


def tiny(name):
    return torch.load(os.path.join(GOLDEN_DIR, 't5_tiny.pt'), weights_only=True)[name]


def cfg_kw(cfg):
    return dict(num_heads=cfg['num_heads'], d_kv=cfg['d_kv'], feed_forward_proj=cfg['feed_forward_proj'],
                relative_attention_num_buckets=cfg['relative_attention_num_buckets'],
                relative_attention_max_distance=cfg['relative_attention_max_distance'], layer_norm_epsilon=cfg['layer_norm_epsilon'])


def restated_kw(cfg, dtype):
    return dict(heads=cfg['num_heads'], gated=cfg['feed_forward_proj'] == 'gated-gelu', num_buckets=cfg['relative_attention_num_buckets'],
                max_distance=cfg['relative_attention_max_distance'], eps=cfg['layer_norm_epsilon'], dtype=dtype)


def ragged_mask(lengths, T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(torch.long)


# ---------------------------------------------------------------- embedding gather
@pytest.mark.parametrize('D, B, T', [(768, 3, 17), (40, 2, 33), (512, 1, 1)])
def test_embedding_gather_is_exact(D, B, T):
    table = rnd(97, D, seed=D)
    ids = torch.randint(0, 97, (B, T), generator=torch.Generator().manual_seed(T))
    y = OPS().t5_embed(ids.to(dev()), table.to(dev()))
    assert y.shape == (D, B * T)
    assert torch.equal(y.cpu(), table[ids.reshape(-1)].t())


def test_embedding_gather_reports_a_bad_id_and_never_reads_it():
    ops = OPS()
    ops.check_device_errors(dev())
    table = rnd(10, 64, seed=1).to(dev())
    ids = torch.tensor([[3, 10, 0, -1, 9, 1 << 40]], dtype=torch.long, device=dev())
    y = ops.t5_embed(ids, table)
    torch.cuda.synchronize()
    assert bool((y[:, [1, 3, 5]] == 0).all()) and torch.equal(y[:, [0, 2, 4]].t(), table[[3, 0, 9]])
    with pytest.raises(IndexError):
        ops.check_device_errors(dev())
    ops.check_device_errors(dev())                                   # the word is cleared by the check


def test_error_word_first_used_under_inference_mode_serves_later_lookups():
    """_condition() runs the encoder under torch.inference_mode(): when that is the first embedding lookup of the process, the device error word and
    its pinned host copy are created there, and the lookups of the training step (outside inference mode) must still be able to poll and clear them"""
    ops = OPS()
    ops.check_device_errors(dev())
    saved = dict(ops._err_flags), dict(ops._err_poll)
    ops._err_flags.clear()
    ops._err_poll.clear()
    try:
        table, ids = rnd(10, 64, seed=1).to(dev()), torch.tensor([[3, 0, 9]], device=dev())
        with torch.inference_mode():
            ops.t5_embed(ids, table)
        for _ in range(3):
            ops.t5_embed(ids, table)
            torch.cuda.synchronize()
        ops.t5_embed(torch.tensor([[11]], device=dev()), table)
        with pytest.raises(IndexError):
            ops.check_device_errors(dev())
    finally:
        ops._err_flags.clear()
        ops._err_poll.clear()
        ops._err_flags.update(saved[0])
        ops._err_poll.update(saved[1])


# ---------------------------------------------------------------- T5LayerNorm
@pytest.mark.parametrize('C', [512, 768, 40])
@pytest.mark.parametrize('N', [1, 70])
def test_rmsnorm_plain_masked_and_transposed(C, N):
    x, w = rnd(C, N, seed=C + N) * 2 + 0.5, 1 + rnd(C, seed=1, scale=0.1)
    mask = (torch.rand(N, generator=torch.Generator().manual_seed(3)) > 0.3).to(torch.uint8)
    xd = x.double()
    want = w.double()[:, None] * (xd * torch.rsqrt(xd.pow(2).mean(0, keepdim=True) + 1e-6))
    tol = (C / 64 + 17 + 8) * U * want.abs() + 1e-30
    ops = OPS()
    xg, wg, mg = x.to(dev()), w.to(dev()), mask.to(dev())
    y = ops.t5_rmsnorm(xg, wg, 1e-6)
    assert y.shape == (C, N)
    check(y, want, tol, f'rmsnorm C{C} N{N}')
    ym = ops.t5_rmsnorm(xg, wg, 1e-6, mask=mg)
    assert torch.equal(ym[:, mask.bool()], y[:, mask.bool()])
    gone = ym[:, ~mask.bool()].cpu()
    assert bool((gone == 0).all()) and not bool(torch.signbit(gone).any())          # exact +0.0
    yt = ops.t5_rmsnorm(xg, wg, 1e-6, transpose_out=True)
    assert yt.shape == (N, C) and torch.equal(yt, y.t())                             # the same arithmetic, written (n, c)
    ytm = ops.t5_rmsnorm(xg, wg, 1e-6, mask=mg, transpose_out=True)
    assert torch.equal(ytm, ym.t())


def test_rmsnorm_masked_columns_are_zero_whatever_they_hold():
    x = rnd(64, 40, seed=5)
    x[:, 3], x[:, 7] = float('nan'), float('inf')
    mask = torch.ones(40, dtype=torch.uint8)
    mask[3] = mask[7] = 0
    for tr in (False, True):
        y = OPS().t5_rmsnorm(x.to(dev()), torch.ones(64, device=dev()), 1e-6, mask=mask.to(dev()), transpose_out=tr)
        y = y.t() if tr else y
        assert bool(torch.isfinite(y).all()) and bool((y[:, [3, 7]] == 0).all())


# ---------------------------------------------------------------- feed-forward gate
def test_gate_gelu_new():
    Fd, N = 96, 53
    x = torch.cat([rnd(Fd, N, seed=1, scale=3.0), rnd(Fd, N, seed=2)])
    x[0, :8] = torch.tensor([0., -0., 1e-20, -1e-20, 12., -12., 40., -40.])
    y = OPS().t5_gate(x.to(dev()), True)
    a, b = x[:Fd].double(), x[Fd:].double()
    g = TR.gelu_new(a)
    assert y.shape == (Fd, N)
    check(y, g * b, b.abs() * 8 * U * (a.abs() + g.abs()) + 1e-37, 'gate gelu_new')


def test_gate_relu_is_exact():
    x = rnd(70, 33, seed=3)
    assert torch.equal(OPS().t5_gate(x.to(dev()), False).cpu(), torch.relu(x))


# ---------------------------------------------------------------- attention: bias, key mask, sample offsets
@pytest.mark.parametrize('T', [1, 31, 32, 33, 64, 65, 200, 256, 300])
def test_attention_bias_and_mask(T):
    B, H = 5, 2
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(3 * H * 64, B * T, generator=g)
    qkv[:2 * H * 64] *= 0.4                                          # q . k over 64 terms: std ~ 1.3, no 1 / sqrt(d) scale in T5
    table = torch.randn(H, 2 * T - 1, generator=g)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 1:] = False                                              # one valid token
    mask[2, max(1, T // 2):] = False                                 # a prefix
    mask[3] = torch.rand(T, generator=g) > 0.4                       # not a prefix
    mask[3, T - 1] = True
    mask[4] = False                                                  # nothing valid: zeros, no NaN
    v3 = qkv[2 * H * 64:].view(H * 64, B, T)
    v3[:, ~mask] = 1e30                                              # a masked key with any probability at all would show
    got = OPS().t5_attn(qkv.to(dev()), table.to(dev()), mask.to(torch.uint8).to(dev()), B, H)
    assert got.shape == (H * 64, B * T) and bool(torch.isfinite(got).all())
    got = got.view(H, 64, B, T).permute(2, 0, 3, 1).cpu().double()   # [B, H, T, 64]
    q, k, v = (t.double().view(H, 64, B, T).permute(2, 0, 3, 1) for t in qkv.view(3, H * 64, B * T))
    i = torch.arange(T)
    bias = table.double()[:, (i[None, :] - i[:, None]) + T - 1]      # [H, i, j]
    s = q @ k.transpose(-1, -2) + bias[None]
    ds = 66 * U * (q.abs() @ k.abs().transpose(-1, -2)) + 2 * U * s.abs()
    key = mask[:, None, None, :]
    s = s.masked_fill(~key, float('-inf'))
    vz = v.masked_fill(~mask[:, None, :, None], 0.)
    rows = mask.any(-1)
    assert rows.tolist() == [True, True, True, True, False]
    p = torch.softmax(s[rows], dim=-1)
    want = p @ vz[rows]
    spread = (s[rows].amax(-1, keepdim=True) - s[rows]).masked_fill(~key[rows], 0.).amax(-1, keepdim=True)
    dsm = ds[rows].masked_fill(~key[rows], 0.).amax(-1, keepdim=True)
    tiles = (T + 31) // 32
    tol = (4 * dsm + 2 * U * spread + (T + 4 * tiles + 16) * U) * (p @ vz[rows].abs()) + 1e-30
    check(got[rows], want, tol, f'attention T{T}')
    assert bool((got[~rows] == 0).all())                             # the all-masked sample
    # the worst-case bound above is loose by two orders of magnitude; the typical-case check is the whole-model rule applied to this kernel: the
    # per-query L2 error relative to the output's norm, maximum over queries, at most 8 x that of the same formula in fp32 on the CPU (and never
    # asked to be below one rounding of the result, u)
    s32 = (q.float() @ k.float().transpose(-1, -2) + bias.float()[None]).masked_fill(~key, float('-inf'))
    cpu32 = (torch.softmax(s32[rows], dim=-1) @ vz[rows].float()).double()
    rel = lambda t: float(((t - want).norm(dim=-1) / want.norm(dim=-1).clamp_min(1e-30)).max())                      # noqa: E731
    r_nat, r_cpu = rel(got[rows]), rel(cpu32)
    print(f'attention T{T}: r_nat {r_nat:.3e}  r_cpu {r_cpu:.3e}')
    assert r_nat <= 8 * max(r_cpu, U), (T, r_nat, r_cpu)


def test_attention_without_a_mask_and_unsupported_head_width():
    from audiolm_pytorch_amd import _lib
    B, H, T = 2, 3, 45
    qkv, table = rnd(3 * H * 64, B * T, seed=1, scale=0.5), rnd(H, 2 * T - 1, seed=2)
    ops = OPS()
    a = ops.t5_attn(qkv.to(dev()), table.to(dev()), None, B, H)
    b = ops.t5_attn(qkv.to(dev()), table.to(dev()), torch.ones(B, T, dtype=torch.uint8, device=dev()), B, H)
    assert torch.equal(a, b)
    with pytest.raises(_lib.AlmError):
        ops.t5_attn(rnd(3 * 2 * 128, 8).to(dev()), rnd(2, 7).to(dev()), None, 2, 2, dim_head=128)


@pytest.mark.parametrize('T', [1, 32, 33, 129])
def test_biased_attention_with_nothing_to_add_is_the_plain_kernel(T):
    """the two attention entry points are one kernel (csrc/dense_f32.hip): with a zero bias table and no key masked, t5_attn gives the bits of
    mha_attn.  Q times 0.125 is exact on the host (a power of two), so every matrix-core operand is the same; s + 0.0 changes at most the sign of a
    zero score, which cannot reach exp(s - max); no tile is skipped and every row sum is positive.  One tile, a tile boundary, a ragged tail,
    more than one 128-query block."""
    B, H = 2, 2
    D = H * 64
    qkv = rnd(B, 3 * D, T, seed=T)
    ops = OPS()
    plain = ops.mha_attn(qkv.to(dev()), H, scale=0.125)
    scaled = qkv.clone()
    scaled[:, :D] *= 0.125
    cn = scaled.permute(1, 0, 2).reshape(3 * D, B * T).contiguous().to(dev())
    zeros = torch.zeros(H, 2 * T - 1, device=dev())
    for mask in (None, torch.ones(B, T, dtype=torch.uint8, device=dev())):
        got = ops.t5_attn(cn, zeros, mask, B, H).view(D, B, T).permute(1, 0, 2)
        assert torch.equal(got, plain), (T, mask is None)


# ---------------------------------------------------------------- whole model
def rel_l2(got, want, valid):
    return float(((got.double() - want).norm(dim=-1)[valid] / want.norm(dim=-1)[valid]).max())


def whole_model_case(sd, kw, rkw, ids, mask, what):
    enc = A().T5Encoder.from_state_dict(sd, **kw).to(dev())
    got = enc(ids.to(dev()), mask.to(dev()))
    want = TR.encode(sd, ids, mask, **{**rkw, 'dtype': F64})
    cpu32 = TR.encode(sd, ids, mask, **{**rkw, 'dtype': torch.float32})
    valid = mask.bool()
    r_nat, r_cpu = rel_l2(got.cpu(), want, valid), rel_l2(cpu32, want, valid)
    print(f'{what}: r_nat {r_nat:.3e}  r_cpu {r_cpu:.3e}  ratio {r_nat / r_cpu:.2f}  (value scale {float(want[valid].abs().max()):.2f})')
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all())
    assert bool((got[~valid.to(dev())] == 0).all())
    assert r_nat <= 8 * r_cpu, (what, r_nat, r_cpu)
    return enc, got


@pytest.mark.parametrize('B, T, lengths', [(8, 256, [256, 1, 17, 100, 255, 33, 64, 200]), (3, 17, [17, 5, 1])])
def test_whole_model_base_size(B, T, lengths):
    sd = TR.random_state_dict(11)                                    # 768 wide, 12 blocks, 12 heads, d_ff 2048, gated-gelu: t5-v1_1-base
    ids = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(B))
    mask = ragged_mask(lengths, T)
    whole_model_case(sd, dict(num_heads=12), dict(heads=12, gated=True), ids, mask, f'v1.1-base size {B} x {T}')


@pytest.mark.parametrize('name', ['gated', 'relu'])
def test_recorded_transformers_forward(name):
    t = tiny(name)
    cfg = t['config']
    enc = A().T5Encoder.from_state_dict(t['state_dict'], **cfg_kw(cfg)).to(dev())
    got = enc(t['ids'].to(dev()), t['mask'].to(dev())).cpu()
    valid = t['mask'].bool()
    cpu32 = TR.encode(t['state_dict'], t['ids'], t['mask'], **restated_kw(cfg, torch.float32))
    r_nat, r_cpu = rel_l2(got, t['output64'], valid), rel_l2(cpu32, t['output64'], valid)
    print(f'recorded {name}: r_nat {r_nat:.3e}  r_cpu {r_cpu:.3e}  ratio {r_nat / r_cpu:.2f}')
    assert bool(torch.isfinite(got).all()) and bool((got[~valid] == 0).all())
    assert r_nat <= 8 * r_cpu, (name, r_nat, r_cpu)


def test_runs_are_bitwise_equal_and_rows_do_not_see_each_other():
    sd = TR.random_state_dict(5, d_model=256, layers=3, heads=4, d_ff=512, vocab=100)
    enc = A().T5Encoder.from_state_dict(sd, num_heads=4).to(dev())
    B, T = 5, 77
    ids = torch.randint(0, 100, (B, T), generator=torch.Generator().manual_seed(1)).to(dev())
    mask = ragged_mask([77, 1, 40, 64, 33], T).to(dev())
    a, b = enc(ids, mask), enc(ids, mask)
    assert torch.equal(a, b)
    for r in range(B):                                               # the same padded length, alone: the same bits
        assert torch.equal(enc(ids[r:r + 1], mask[r:r + 1])[0], a[r]), r
    full = enc(ids)                                                  # no mask = a mask of ones
    assert torch.equal(full, enc(ids, torch.ones_like(mask)))


# ---------------------------------------------------------------- end to end: text= on the transformers
@pytest.fixture
def registered():
    t = tiny('gated')
    a = A()
    enc = a.T5Encoder.from_state_dict(t['state_dict'], **cfg_kw(t['config'])).to(dev())
    tok = TR.StubTokenizer(t['config']['vocab_size'])
    a.register_t5(NAME, enc, tok)
    try:
        yield t, enc, tok
    finally:
        from audiolm_pytorch_amd import t5
        t5.unregister_t5(NAME)


class Codec:
    """what CoarseTransformerWrapper reads of a codec when it is handed token ids"""
    rq_groups, num_quantizers, codebook_size = 1, 8, 40


TEXTS = ['a dog barking in the rain', 'rain', 'slow piano over a distant city at night with wind']


def test_t5_encode_text_is_the_masked_restated_forward(registered):
    t, enc, tok = registered
    got = A().t5_encode_text(TEXTS, name=NAME)
    e = tok(TEXTS, return_tensors='pt', padding='longest', max_length=256, truncation=True)
    assert got.shape == (3, e.input_ids.shape[1], 64) and got.is_cuda
    want = TR.encode(t['state_dict'], e.input_ids, e.attention_mask, **restated_kw(t['config'], F64))
    cpu32 = TR.encode(t['state_dict'], e.input_ids, e.attention_mask, **restated_kw(t['config'], torch.float32))
    valid = e.attention_mask.bool()
    assert rel_l2(got.cpu(), want, valid) <= 8 * rel_l2(cpu32, want, valid)
    assert bool((got.cpu()[~valid] == 0).all())
    one = A().t5_encode_text(TEXTS[1], name=NAME)                    # a bare string is one text
    assert one.shape == (1, 2, 64)


def test_coarse_text_equals_text_embeds_bitwise(registered):
    a = A()
    torch.manual_seed(0)
    m = a.CoarseTransformer(dim=128, depth=2, num_semantic_tokens=30, codebook_size=40, num_coarse_quantizers=3, has_condition=True,
                            t5_name=NAME).to(dev()).eval()
    assert tuple(m.proj_text_embed.weight.shape) == (128, 64)
    g = torch.Generator().manual_seed(2)
    sem, coarse = torch.randint(0, 30, (3, 7), generator=g).to(dev()), torch.randint(0, 40, (3, 6), generator=g).to(dev())
    with torch.no_grad():
        s1, c1 = m(semantic_token_ids=sem, coarse_token_ids=coarse, text=TEXTS, cond_drop_prob=0.)
        s2, c2 = m(semantic_token_ids=sem, coarse_token_ids=coarse, text_embeds=a.t5_encode_text(TEXTS, name=NAME), cond_drop_prob=0.)
    assert torch.equal(s1, s2) and torch.equal(c1, c2) and bool(torch.isfinite(c1).all())


def test_coarse_text_trains(registered):
    """text= inside a training step, as the reference trainers call the wrapper: the loss back-propagates into proj_text_embed (the encoder is frozen)"""
    a = A()
    torch.manual_seed(0)
    m = a.CoarseTransformer(dim=128, depth=2, num_semantic_tokens=30, codebook_size=40, num_coarse_quantizers=3, has_condition=True,
                            t5_name=NAME).to(dev()).train()
    g = torch.Generator().manual_seed(2)
    sem, coarse = torch.randint(0, 30, (3, 7), generator=g).to(dev()), torch.randint(0, 40, (3, 6), generator=g).to(dev())
    w = a.CoarseTransformerWrapper(transformer=m, codec=Codec(), unique_consecutive=False).train()
    loss = w(semantic_token_ids=sem, coarse_token_ids=coarse.view(3, 2, 3), text=TEXTS, cond_drop_prob=0., return_loss=True)     # the trainers' call
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(m.proj_text_embed.weight.grad.norm()) > 0


def test_semantic_ragged_text_matches_the_oracle_with_the_token_mask(registered):
    """SemanticTransformer derives the context mask from the embeddings only when it ran the encoder itself (reference :692-695): with text= the
    padded text positions are masked.  Oracle: the restated encoder's embeddings as context, the tokenizer's mask as context_mask; bound: the
    1.5e-2 relative Frobenius error of the existing masked-conditioning test (tests/test_gpu_bias.py)."""
    import audiolm_oracle as O
    from common import synth_state_dict
    t, enc, tok = registered
    a = A()
    m = a.SemanticTransformer(dim=128, depth=2, num_semantic_tokens=30, heads=4, has_condition=True, t5_name=NAME, flash_attn=True)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 91)
    m.load_state_dict(sd)
    m.to(dev()).eval()
    ids = torch.randint(0, 30, (3, 9), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        got = m(ids=ids.to(dev()), text=TEXTS, cond_drop_prob=0.)
    e = tok(TEXTS, return_tensors='pt', padding='longest', max_length=256, truncation=True)
    assert not bool(e.attention_mask.all())                          # the texts are ragged
    te = TR.encode(t['state_dict'], e.input_ids, e.attention_mask, **restated_kw(t['config'], torch.float32))
    tokens = torch.cat((sd['start_token'].expand(3, 1, -1), O.get_embeds(sd['semantic_embedding.weight'], ids)), dim=1)
    h = O.transformer(sd, 'transformer.', tokens, depth=2, heads=4, streams=4, context=F.linear(te, sd['proj_text_embed.weight']),
                      context_mask=e.attention_mask.bool())
    want = O.head_linear(h, sd['to_logits.weight'], sd['to_logits.bias'])
    err = float((got.cpu().double() - want.double()).norm() / want.double().norm())
    print(f'semantic text= vs oracle: rel-frob {err:.3e}')
    assert got.shape == want.shape and err <= 1.5e-2, err


def test_guided_forward_and_generate_from_text(registered):
    t, enc, tok = registered
    a = A()
    torch.manual_seed(0)
    m = a.SemanticTransformer(dim=64, depth=2, num_semantic_tokens=30, has_condition=True, t5_name=NAME, flash_attn=True).to(dev()).eval()
    ids = torch.randint(0, 30, (3, 5), generator=torch.Generator().manual_seed(1)).to(dev())
    with torch.no_grad():
        lg = m.forward_with_cond_scale(ids=ids, text=TEXTS, cond_scale=3)
    assert lg.shape == (3, 6, 31) and bool(torch.isfinite(lg).all())
    w = a.SemanticTransformerWrapper(transformer=m, unique_consecutive=False)
    for cache in (True, False):
        before = tok.calls
        out = w.generate(max_length=8, batch_size=3, text=TEXTS, cond_scale=3., use_kv_cache=cache)
        assert tok.calls == before + 1                               # encoded once per sampling run
        assert out.shape[0] == 3 and out.dtype == torch.long and int(out.max()) <= 30 and int(out.min()) >= -1
    mc = a.CoarseTransformer(dim=64, depth=2, num_semantic_tokens=30, codebook_size=40, num_coarse_quantizers=3, has_condition=True,
                             t5_name=NAME).to(dev()).eval()
    wc = a.CoarseTransformerWrapper(transformer=mc, codec=Codec(), unique_consecutive=False)
    before = tok.calls
    sem = torch.randint(0, 30, (3, 6), generator=torch.Generator().manual_seed(3)).to(dev())
    out = wc.generate(semantic_token_ids=sem, max_time_steps=2, text=TEXTS, cond_scale=3.)
    assert tok.calls == before + 1
    assert out.shape[0] == 3 and int(out.max()) <= 40 and int(out.min()) >= -1
