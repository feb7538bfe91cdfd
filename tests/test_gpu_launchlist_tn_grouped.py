"""MI355X: a recorded launch list carries the grouped weight-gradient leftovers (alm_gemm_bf16_tn_batched_panels + alm_gemm_bf16_tn_grouped): the job
table is a host array whose pointer words the recorder places against the bases of the pass like any pointer argument.  Same bar as
tests/test_gpu_launchlist.py: a replayed step is `torch.equal` to the step issued launch by launch from Python (depth loop and autograd of reference
audiolm_pytorch.py:528-547)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class Codec:
    rq_groups = 1
    num_quantizers = 8


def _step(model, w, kw):
    torch.manual_seed(1)
    for p in model.parameters():
        p.grad = None
    with torch.autocast('cuda', dtype=torch.bfloat16):
        loss = w(**kw, return_loss=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_depth2_stack_replays_the_grouped_launch_bitwise(monkeypatch):
    import audiolm_pytorch_amd as A
    from audiolm_pytorch_amd import launchlist as LL, ops
    assert ops.TN_GROUPED, 'the grouped leftover launch is switched off (ALM_TN_GROUPED=0)'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = A.CoarseTransformer(dim=256, depth=2, heads=4, num_semantic_tokens=50, codebook_size=64, num_coarse_quantizers=3, flash_attn=True).to(dev)
    w = A.CoarseTransformerWrapper(transformer=m, codec=Codec(), unique_consecutive=False, mask_prob=0.15)
    w.train()
    g = torch.Generator().manual_seed(3)
    kw = dict(semantic_token_ids=torch.randint(0, 50, (2, 96), generator=g).to(dev), coarse_token_ids=torch.randint(0, 64, (2, 96, 3), generator=g).to(dev))
    calls = []
    real = ops.gemm_tn_grouped
    monkeypatch.setattr(ops, 'gemm_tn_grouped', lambda left, slices=0: (calls.append(len(left)), real(left, slices))[1])
    monkeypatch.setattr(LL, 'ENABLED', False)
    eager = _step(m, w, kw)
    assert calls == [5], calls                                  # one grouped launch for the five weight kinds of the stack
    monkeypatch.setattr(LL, 'ENABLED', True)
    LL.PLANS.clear()
    before = dict(LL.STATS)
    steps = [_step(m, w, kw) for _ in range(4)]                 # size, record, replay, replay
    assert LL.STATS['refused'] == before['refused'], [p.why for p in LL.PLANS.values()]
    assert LL.STATS['recorded'] - before['recorded'] == 2 and LL.STATS['replayed'] - before['replayed'] == 2
    assert len(calls) == 3                                      # the replays issue it from the list, not from Python
    names = [n for p in LL.PLANS.values() if p.bwd is not None for n in p.bwd.names]
    assert names.count('alm_gemm_bf16_tn_grouped') == 1 and names.count('alm_gemm_bf16_tn_batched_panels') == 5 and 'alm_gemm_bf16_tn_batched' not in names
    for other in steps:
        assert torch.equal(eager[0], other[0])
        assert eager[1].keys() == other[1].keys() and len(eager[1]) > 20
        bad = [k for k in eager[1] if not torch.equal(eager[1][k], other[1][k])]
        assert not bad, bad[:8]
