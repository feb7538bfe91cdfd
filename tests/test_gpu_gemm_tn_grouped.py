"""MI355X: the grouped leftover launch of the batched weight gradients (alm_gemm_bf16_tn_batched_panels + alm_gemm_bf16_tn_grouped, csrc/gemm.hip).

dW = dY^T X over K = tokens (autograd of every nn.Linear of the stack, reference audiolm_pytorch.py:255-259, :351, :395): the tiles of several weight kinds
that do not fill whole rounds of the chip run as ONE launch of uniform K slices and one fixed-order reduce.  Inputs are random bf16 in [-1, 1), the
reference is an fp64 matmul of the same bf16 values, the bound is the one of the existing TN split-K cases (tests/test_gpu_kernels.py: relmax <= 2e-5)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
BOUND = 2e-5


@pytest.fixture(scope='module')
def ops():
    import audiolm_pytorch_amd  # noqa: F401
    from audiolm_pytorch_amd import ops as o
    return o


def dev():
    return torch.device('cuda:0')


def uni(*shape, seed=0, dtype=BF16):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(dev()).to(dtype)


def relmax(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


K_MIXED = 1096                                                  # 18 K-steps of 64, the last one 8 deep: uneven last slices
SHAPES = ((512, 1024, 2), (128, 1024, 2), (600, 520, 1))        # (M, N, nb): whole tiles; a half-empty tile; ragged in both dimensions


@pytest.fixture(scope='module')
def mixed():
    """operands of the mixed group, the starting C of every job and the fp64 reference (alpha 0.5 everywhere, accumulate on the last job)"""
    out = []
    for i, (M, N, nb) in enumerate(SHAPES):
        At, Bt = uni(1, nb, K_MIXED, M, seed=10 + i), uni(1, nb, K_MIXED, N, seed=20 + i)
        C0 = uni(1, nb, M, N, seed=30 + i, dtype=F32)
        acc = i == 2
        ref = 0.5 * torch.einsum('lhkm,lhkn->lhmn', At.double(), Bt.double()) + (C0.double() if acc else 0.)
        out.append((At, Bt, C0, acc, ref))
    return out


def run_mixed(ops, mixed, slices):
    Cs = [C0.clone() for _, _, C0, _, _ in mixed]
    jobs = [ops.tn_job(At, Bt, C, alpha=0.5, accumulate=acc) for (At, Bt, _, acc, _), C in zip(mixed, Cs)]
    ops.gemm_tn_grouped(jobs, slices=slices)
    torch.cuda.synchronize()
    return Cs, jobs


@pytest.mark.parametrize('slices', [1, 0, 2, 4])                # forced single slice (no partials, no reduce); the planned count; forced splits (9 + 9, 5 + 5 + 5 + 3 K-steps)
def test_mixed_group_matches_fp64(ops, mixed, slices):
    Cs, jobs = run_mixed(ops, mixed, slices)
    plan = ops.gemm_tn_grouped_plan(jobs, slices)
    assert plan[0] == 2 * 4 * 2 + 1 * 4 * 2 + 3 * 3 and plan[3] == plan[0] * plan[1]
    if slices:
        assert plan[1] == slices
    for C, (_, _, _, _, ref) in zip(Cs, mixed):
        err = relmax(C, ref)
        print(f'slices={slices} planned={plan[1]} relmax={err:.3e}')
        assert err <= BOUND, err


def test_two_calls_are_bitwise_equal(ops, mixed):
    for slices in (0, 4):
        a, _ = run_mixed(ops, mixed, slices)
        b, _ = run_mixed(ops, mixed, slices)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('K', [4096, 128])
def test_panels_plus_grouped_equals_batched(ops, K):
    """M = 17 tile rows x N = 16 tile columns, one problem: 272 tiles.  K = 4096 is the shortest contraction for which the hybrid plan has whole rounds
    (16 panels = 256 tiles at full K; the 17th tile row is the tail descriptor): those tiles must be bitwise alm_gemm_bf16_tn_batched's.  K = 128: the plan
    has no whole round, the descriptor is the whole problem and nothing is launched before the grouped call."""
    from audiolm_pytorch_amd import _lib
    M, N = 4096 + 256, 4096
    plan = (ctypes.c_int * 4)()
    kind = _lib.query('alm_gemm_tn_batched_plan', M, N, K, 1, ctypes.cast(plan, ctypes.c_void_p))
    At, Bt = uni(1, 1, K, M, seed=41), uni(1, 1, K, N, seed=42)
    full = torch.empty((1, 1, M, N), dtype=F32, device=dev())
    ops.gemm_tn_batched(At, Bt, full, alpha=0.5)
    C = torch.full((1, 1, M, N), float('nan'), dtype=F32, device=dev())
    left = []
    ops.gemm_tn_batched(At, Bt, C, alpha=0.5, leftovers=left)
    assert len(left) == 1
    rest = left[0][0][0]
    if K >= 4096:
        assert kind == 2 and list(plan)[0] == 16 and plan[2] == 4096 and plan[3] == 1
        assert (rest.M, rest.N, rest.nb1, rest.nb2) == (256, N, 1, 1) and rest.C == C.data_ptr() + 4096 * N * 4 and rest.At == At.data_ptr() + 4096 * 2
        torch.cuda.synchronize()
        assert torch.equal(C[0, 0, :4096], full[0, 0, :4096])               # the whole-round tiles: the same kernel, the same bits
        assert bool(torch.isnan(C[0, 0, 4096:]).all())                       # the tail: not launched yet
    else:
        assert kind != 2 and (rest.M, rest.N) == (M, N) and rest.C == C.data_ptr()
        torch.cuda.synchronize()
        assert bool(torch.isnan(C).all())
    ops.gemm_tn_grouped(left)
    torch.cuda.synchronize()
    ref = 0.5 * (At[0, 0].double().t() @ Bt[0, 0].double())
    err, err_full = relmax(C[0, 0], ref), relmax(full[0, 0], ref)
    print(f'K={K} relmax grouped={err:.3e} batched={err_full:.3e} vs each other={relmax(C, full):.3e}')
    assert err <= BOUND and relmax(C, full) <= BOUND
    if K >= 4096:
        assert torch.equal(C[0, 0, :4096], full[0, 0, :4096])


def test_plan_of_the_headline_leftovers():
    """the five weight kinds of the headline step (K = 16384 tokens, 6 layers, dim 1024, inner 2730, 8 heads of 64): the tails of dW1 / dW2 as
    alm_gemm_tn_batched_plan cuts them + dWo, dWq, dWkv whole.  Host arithmetic only (the pointers are never dereferenced)."""
    from audiolm_pytorch_amd import _lib
    K, L, D, I = 16384, 6, 1024, 2730
    plan4 = (ctypes.c_int * 4)()
    assert _lib.query('alm_gemm_tn_batched_plan', I, D, K, 2 * L, ctypes.cast(plan4, ctypes.c_void_p)) == 2 and plan4[3] == 1
    m1 = I - plan4[2]
    assert _lib.query('alm_gemm_tn_batched_plan', D, I, K, L, ctypes.cast(plan4, ctypes.c_void_p)) == 2 and plan4[3] == 0
    n2 = I - plan4[2]
    shapes = [(m1, D, 1), (D, n2, 1), (D, 512, L), (512, D, L), (128, D, L)]
    jobs = (_lib.AlmTnJob * len(shapes))()
    for j, (M, N, nb) in zip(jobs, shapes):
        j.At, j.Bt, j.C, j.M, j.N, j.K, j.nb1, j.nb2, j.alpha = 0x100000, 0x200000, 0x300000, M, N, K, nb, 1, 1.0
        j.lda, j.ldb, j.ldc, j.sA1, j.sB1, j.sC1 = 2736 * 2, 2736, N, K * 2736 * 2, K * 2736, M * N
    plan = (ctypes.c_int * 6)()
    S = _lib.query('alm_gemm_tn_grouped_plan', jobs, len(shapes), 0, ctypes.cast(plan, ctypes.c_void_p))
    tiles, s_, kps, pieces, blocks, rounds = plan
    print('headline leftovers: plan', list(plan))
    assert tiles == sum(-(-M // 256) * -(-N // 256) * nb for M, N, nb in shapes) == 16 + 8 + 48 + 48 + 24
    ksteps = K // 64
    assert S == s_ >= 1 and S * kps >= ksteps > (S - 1) * kps                # slice s covers K-steps [s kps, (s + 1) kps): each step once, no empty slice
    assert pieces == tiles * S
    assert blocks % 8 == 0 and blocks >= pieces and rounds == -(-(blocks // 8) // 32)
    assert blocks - pieces < 8 * 16 * len(shapes)                           # the XCD lists differ by at most one unit (<= 16 tiles) per job
    need = S * sum(M * N * nb for M, N, nb in shapes) if S > 1 else 0
    assert _lib.query('alm_gemm_tn_grouped_ws_floats', jobs, len(shapes), 0) >= need
    for forced in (1, 3, 7):
        assert _lib.query('alm_gemm_tn_grouped_plan', jobs, len(shapes), forced, ctypes.cast(plan, ctypes.c_void_p)) == forced
        assert plan[3] == tiles * forced and forced * plan[2] >= ksteps > (forced - 1) * plan[2]
        assert _lib.query('alm_gemm_tn_grouped_ws_floats', jobs, len(shapes), forced) >= (forced * sum(M * N * nb for M, N, nb in shapes) if forced > 1 else 0)
    jobs[1].K = K - 64                                                       # two contraction lengths in one call: refused
    assert _lib.query('alm_gemm_tn_grouped_plan', jobs, len(shapes), 0, None) < 0
