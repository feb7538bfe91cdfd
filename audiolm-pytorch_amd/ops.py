"""Thin tensor-level wrappers over the C ABI (one Python function per `alm_*` entry).  PyTorch only supplies device
memory and the stream; all arithmetic happens in libaudiolm_hip.so.  No CPU / eager fallback exists on purpose.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _lib

BF16, F32 = torch.bfloat16, torch.float32


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
# current device as ONE C call (torch.cuda.current_device() is a Python wrapper with a lazy-init check: ~0.9 us, and _chk / _st run ~600 times per step)
_cur_dev = getattr(torch._C, '_cuda_getDevice', None) or torch.cuda.current_device


def _st():
    """hipStream_t of torch's CURRENT stream on the current device (every alm_* launch goes there).  The raw-handle query is one C call; the
    public torch.cuda.current_stream() builds a Stream object per call (~8 us: ~1.5 ms of host time per training step at ~180 launches)."""
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype=None):
    if not t.is_cuda:
        raise _lib.AlmError('audiolm_pytorch_amd ops run on the MI355X only (got a CPU tensor); there is no CPU fallback')
    if dtype is not None and t.dtype != dtype:
        raise _lib.AlmError(f'expected {dtype}, got {t.dtype}')
    if t.device.index != _cur_dev():
        # every launch goes to the CURRENT device's stream (_st): a tensor of another device would be dereferenced there
        raise _lib.AlmError(f'tensor on cuda:{t.device.index} but the current device is cuda:{torch.cuda.current_device()}: call '
                            'torch.cuda.set_device(...) (one process per GPU) before using audiolm_pytorch_amd')
    return t


def _p(t):
    return None if t is None else t.data_ptr()


# Every device buffer an op wrapper creates goes through _new / _new_zeros / _new_like.  ALLOC is None in ordinary use (torch's caching allocator); while
# launchlist.py sizes or records a stack pass it is an allocator object (a byte tally / a bump allocator over the pass's arena), so that every temporary of
# the pass sits at a fixed offset of ONE buffer and the recorded launch list can be re-issued against a fresh arena.
ALLOC = None


def _new(shape, dtype=None, device=None):
    if ALLOC is not None:
        return ALLOC.empty(shape, dtype, device)
    return torch.empty(shape, dtype=dtype, device=device)


def _new_zeros(shape, dtype=None, device=None):
    if ALLOC is not None:
        return ALLOC.zeros(shape, dtype, device)
    return torch.zeros(shape, dtype=dtype, device=device)


def _new_like(t):
    if ALLOC is not None and t.is_contiguous():
        return ALLOC.empty(t.shape, t.dtype, t.device)
    return torch.empty_like(t)


def memset_zero(t):
    """zero-fill of a contiguous tensor on the current stream by a kernel (C ABI: alm_memset_zero; not hipMemsetAsync: its small graph nodes replay wrongly)"""
    assert t.is_contiguous()
    _lib.call('alm_memset_zero', t.data_ptr(), t.numel() * t.element_size(), _st())
    return t


def persistent_buffers():
    """device buffers that live at a fixed address for the life of the process (a recorded launch list may carry their addresses as literals)"""
    return list(_NT_WS.values())


def _rows_ld(t):
    """2-D row-major view -> (rows, cols, ld)."""
    assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return t.shape[0], t.shape[1], t.stride(0)


# ------------------------------------------------------------------------------------------------ dense contractions

# Workspace of the in-launch split-K NT launches (alm_gemm_bf16_nt_ws): one persistent buffer per (device, stream) -- a launch owns its slabs and ticket
# counters until it retires, and launches on ONE stream retire in order.  Zeroed once (the counters; every launch leaves them zero).  64 MB + 4 KB.
_NT_WS = {}
NT_WS = os.environ.get('ALM_GEMM_NT_WS', '1') != '0'           # A/B switch: 0 = never hand a workspace over (the round-5 launches)


def _nt_ws(dev, stream):
    key = (dev.index, stream)
    ws = _NT_WS.get(key)
    if ws is None:
        ws = _NT_WS[key] = torch.zeros(_lib.query('alm_gemm_nt_ws_bytes'), dtype=torch.uint8, device=dev)
    return ws


def gemm_nt(A, B, C, *, bias=None, alpha=1.0, accumulate=False):
    """C[..., M, N] (+)= alpha * A[..., M, K] @ B[..., N, K]^T (+ bias).  Up to two leading batch dims (broadcast via stride 0)."""
    _chk(A, BF16), _chk(B, BF16), _chk(C)
    assert A.stride(-1) == 1 and B.stride(-1) == 1 and C.stride(-1) == 1
    nb = A.dim() - 2
    assert nb in (0, 1, 2) and B.dim() == A.dim() and C.dim() == A.dim()
    M, K = A.shape[-2:]
    N = B.shape[-2]
    assert B.shape[-1] == K and C.shape[-2] == M and C.shape[-1] == N, (A.shape, B.shape, C.shape)
    bs = [1, 1]
    sa, sb, sc = [0, 0], [0, 0], [0, 0]
    for i in range(nb):
        j = 2 - nb + i
        bs[j] = A.shape[i]
        sa[j], sb[j], sc[j] = A.stride(i), B.stride(i) if B.shape[i] != 1 else 0, C.stride(i)
    st = _st()
    if NT_WS and M >= 256 and N >= 256:
        ws = _nt_ws(A.device, st)
        _lib.call('alm_gemm_bf16_nt_ws', A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(bias), M, N, K, A.stride(-2), B.stride(-2), C.stride(-2),
                  bs[0], bs[1], sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], float(alpha), int(C.dtype == F32), int(accumulate), ws.data_ptr(), ws.numel(), st)
    else:
        _lib.call('alm_gemm_bf16_nt', A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(bias), M, N, K, A.stride(-2), B.stride(-2), C.stride(-2),
                  bs[0], bs[1], sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], float(alpha), int(C.dtype == F32), int(accumulate), st)
    return C


def gemm_nt_inl(A, B, C, slices, *, bias=None, alpha=1.0, accumulate=False):
    """un-batched gemm_nt on the staggered 256 x 256 tile with a GIVEN number of in-launch K slices (alm_gemm_bf16_nt_inl): tests / benchmarks"""
    _chk(A, BF16), _chk(B, BF16), _chk(C)
    M, K = A.shape
    N = B.shape[0]
    st = _st()
    ws = _nt_ws(A.device, st)
    _lib.call('alm_gemm_bf16_nt_inl', A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(bias), M, N, K, A.stride(0), B.stride(0), C.stride(0),
              float(alpha), int(C.dtype == F32), int(accumulate), int(slices), ws.data_ptr(), ws.numel(), st)
    return C


def gemm_nt_group2(A0, B0, C0, A1, B1, C1):
    """C0 = A0 @ B0^T and C1 = A1 @ B1^T (2-D, last dim contiguous, both outputs of one dtype) in ONE launch when the two problems pick the same block
    tile (alm_gemm_bf16_nt_group2; two launches otherwise -- identical results)."""
    for t in (A0, B0, A1, B1):
        _chk(t, BF16)
        assert t.dim() == 2 and t.stride(1) == 1
    _chk(C0), _chk(C1)
    assert C0.dtype == C1.dtype and C0.stride(1) == 1 and C1.stride(1) == 1
    (M0, K0), (M1, K1), N0, N1 = A0.shape, A1.shape, B0.shape[0], B1.shape[0]
    assert B0.shape[1] == K0 and B1.shape[1] == K1 and tuple(C0.shape) == (M0, N0) and tuple(C1.shape) == (M1, N1)
    _lib.call('alm_gemm_bf16_nt_group2', A0.data_ptr(), B0.data_ptr(), C0.data_ptr(), M0, N0, K0, A0.stride(0), B0.stride(0), C0.stride(0),
              A1.data_ptr(), B1.data_ptr(), C1.data_ptr(), M1, N1, K1, A1.stride(0), B1.stride(0), C1.stride(0), int(C0.dtype == F32), _st())
    return C0, C1


def _splitk(name, A, B, C, M, N, K, nb, sA, sB, sC, alpha, accumulate):
    nws = _lib.query('alm_gemm_splitk_ws_floats', M, N, K, nb)
    if nws < 0:
        raise _lib.AlmError('split-K workspace exceeds 2^31 floats')
    ws = _new(nws, dtype=F32, device=A.device) if nws > 0 else None
    _lib.call(name, A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(ws), M, N, K, A.stride(-2), B.stride(-2), C.stride(-2), nb, sA, sB, sC,
              float(alpha), int(accumulate), _st())
    return C


def gemm_nt_splitk(A, B, C, *, alpha=1.0, accumulate=False):
    """fp32 C[M, N] (+)= alpha * A[M, K] @ B[N, K]^T with K split over workgroups (long-K, few-tile contractions)."""
    _chk(A, BF16), _chk(B, BF16), _chk(C, F32)
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K and C.shape == (M, N) and A.stride(1) == 1 and B.stride(1) == 1 and C.stride(1) == 1
    return _splitk('alm_gemm_bf16_nt_splitk', A, B, C, M, N, K, 1, 0, 0, 0, alpha, accumulate)


def gemm_tn_splitk(At, Bt, C, *, alpha=1.0, accumulate=False):
    """fp32 C[(nb,) M, N] (+)= alpha * At[K, (nb,) M]^T @ Bt[K, N]: the weight-gradient contraction over K = tokens, read straight from
    the row-major activations (LDS transpose reads inside the kernel; no transposed copies).  A 3-D `At` of shape [nb, K, M] (a strided
    view, e.g. the x / gate halves of dU) with a 3-D C [nb, M, N] runs the nb problems in one launch against the same Bt."""
    _chk(At, BF16), _chk(Bt, BF16), _chk(C, F32)
    nb, sA, sC = 1, 0, 0
    if At.dim() == 3:
        nb, sA, sC = At.shape[0], At.stride(0), C.stride(0)
        assert C.dim() == 3 and C.shape[0] == nb
    K, M = At.shape[-2:]
    N = Bt.shape[1]
    assert Bt.dim() == 2 and Bt.shape[0] == K and C.shape[-2:] == (M, N) and At.stride(-1) == 1 and Bt.stride(1) == 1 and C.stride(-1) == 1
    return _splitk('alm_gemm_bf16_tn_splitk', At, Bt, C, M, N, K, nb, sA, 0, sC, alpha, accumulate)


def gemm_tn_batched(At, Bt, C, *, alpha=1.0, accumulate=False, leftovers=None):
    """fp32 C[n1, n2, M, N] (+)= alpha * At[n1, n2, K, M]^T @ Bt[n1, n2, K, N]: 4-D strided views (last dim contiguous; a size-1 / stride-0 leading dim of Bt
    broadcasts), e.g. every layer's gradient of one weight kind from stacked activation buffers in ONE launch.
    leftovers: a list -> only the panels that fill whole rounds of the chip are launched (alm_gemm_bf16_tn_batched_panels) and the job that is left (the
    hybrid plan's tail, or the whole problem) is appended to it: C is complete only after gemm_tn_grouped(leftovers)."""
    _chk(At, BF16), _chk(Bt, BF16), _chk(C, F32)
    assert At.dim() == 4 and Bt.dim() == 4 and C.dim() == 4 and At.stride(-1) == 1 and Bt.stride(-1) == 1 and C.stride(-1) == 1
    n1, n2, K, M = At.shape
    N = Bt.shape[-1]
    assert Bt.shape[-2] == K and tuple(C.shape) == (n1, n2, M, N), (At.shape, Bt.shape, C.shape)
    sb = [Bt.stride(0) if Bt.shape[0] != 1 else 0, Bt.stride(1) if Bt.shape[1] != 1 else 0]
    if leftovers is not None:
        rest = (_lib.AlmTnJob * 1)()
        _lib.call('alm_gemm_bf16_tn_batched_panels', At.data_ptr(), Bt.data_ptr(), C.data_ptr(), M, N, K, At.stride(-2), Bt.stride(-2), C.stride(-2), n1, n2,
                  At.stride(0), At.stride(1), sb[0], sb[1], C.stride(0), C.stride(1), float(alpha), int(accumulate), rest, _st())
        if rest[0].M > 0:
            leftovers.append((rest, At, Bt, C))          # (the tensors: kept alive until the grouped launch is issued)
        return C
    nws = _lib.query('alm_gemm_splitk_ws_floats', M, N, K, n1 * n2)
    if nws < 0:
        raise _lib.AlmError('split-K workspace exceeds 2^31 floats')
    ws = _new(nws, dtype=F32, device=At.device) if nws > 0 else None
    _lib.call('alm_gemm_bf16_tn_batched', At.data_ptr(), Bt.data_ptr(), C.data_ptr(), _p(ws), M, N, K, At.stride(-2), Bt.stride(-2), C.stride(-2), n1, n2,
              At.stride(0), At.stride(1), sb[0], sb[1], C.stride(0), C.stride(1), float(alpha), int(accumulate), _st())
    return C


TN_GROUP_MAX = 8
# The parts of the stack's five batched weight-gradient launches that do not fill whole rounds of the chip are finished by ONE grouped launch (core.stack_backward,
# single group, no gradient hook).  ALM_TN_GROUPED=0: today's per-kind calls (A/B switch; interleaved on one box: 11.72 -> 11.58 ms/step, docs/LABBOOK.md round 7)
TN_GROUPED = os.environ.get('ALM_TN_GROUPED', '1') != '0'


def _tn_jobs(leftovers):
    arr = (_lib.AlmTnJob * len(leftovers))()
    for i, lo in enumerate(leftovers):
        ctypes.memmove(ctypes.byref(arr, i * ctypes.sizeof(_lib.AlmTnJob)), lo[0], ctypes.sizeof(_lib.AlmTnJob))
    return arr


def gemm_tn_grouped_plan(leftovers, slices=0):
    """(tiles, slices, K-steps per slice, pieces, workgroups, rounds) of gemm_tn_grouped(leftovers, slices) -- no launch"""
    plan = (ctypes.c_int * 6)()
    if _lib.query('alm_gemm_tn_grouped_plan', _tn_jobs(leftovers), len(leftovers), int(slices), ctypes.cast(plan, ctypes.c_void_p)) < 0:
        raise _lib.AlmError('alm_gemm_tn_grouped_plan: bad job table')
    return tuple(plan)


def gemm_tn_grouped(leftovers, slices=0):
    """finishes the C of every gemm_tn_batched(..., leftovers=leftovers) call: the jobs' 256 x 256 tiles, cut into ONE number of K slices, in one launch and
    one fixed-order reduce (alm_gemm_bf16_tn_grouped; at most 8 jobs per launch, all of one K).  slices: 0 = the library's cost model."""
    for g0 in range(0, len(leftovers), TN_GROUP_MAX):
        arr = _tn_jobs(leftovers[g0:g0 + TN_GROUP_MAX])
        nws = _lib.query('alm_gemm_tn_grouped_ws_floats', arr, len(arr), int(slices))
        if nws < 0:
            raise _lib.AlmError('alm_gemm_tn_grouped: bad job table, or its split-K workspace exceeds 2^31 floats')
        dev = next(lo[1].device for lo in leftovers[g0:g0 + TN_GROUP_MAX])
        ws = _new(nws, dtype=F32, device=dev) if nws > 0 else None
        _lib.call('alm_gemm_bf16_tn_grouped', arr, len(arr), _p(ws), int(slices), _st())


def tn_job(At, Bt, C, *, alpha=1.0, accumulate=False):
    """a whole gemm_tn_batched problem as a job of gemm_tn_grouped (nothing launched)"""
    _chk(At, BF16), _chk(Bt, BF16), _chk(C, F32)
    assert At.dim() == 4 and Bt.dim() == 4 and C.dim() == 4 and At.stride(-1) == 1 and Bt.stride(-1) == 1 and C.stride(-1) == 1
    n1, n2, K, M = At.shape
    N = Bt.shape[-1]
    assert Bt.shape[-2] == K and tuple(C.shape) == (n1, n2, M, N), (At.shape, Bt.shape, C.shape)
    sb = [Bt.stride(0) if Bt.shape[0] != 1 else 0, Bt.stride(1) if Bt.shape[1] != 1 else 0]
    job = (_lib.AlmTnJob * 1)()
    job[0] = _lib.AlmTnJob(At.data_ptr(), Bt.data_ptr(), C.data_ptr(), M, N, K, n1, n2, int(accumulate), float(alpha), 0, At.stride(-2), Bt.stride(-2),
                           C.stride(-2), At.stride(0), At.stride(1), sb[0], sb[1], C.stride(0), C.stride(1))
    return (job, At, Bt, C)


def gemm_nt_tile(A, B, C, tile, *, bias=None, alpha=1.0, accumulate=False):
    """un-batched gemm_nt with an explicit tile configuration (0 auto, 1 = 128x128, 2 = 256x256): tuning / benchmarks."""
    _chk(A, BF16), _chk(B, BF16), _chk(C)
    M, K = A.shape
    N = B.shape[0]
    _lib.call('alm_gemm_bf16_nt_tile', A.data_ptr(), B.data_ptr(), C.data_ptr(), _p(bias), M, N, K, A.stride(0), B.stride(0), C.stride(0),
              float(alpha), int(C.dtype == F32), int(accumulate), int(tile), _st())
    return C


def transpose(src, rows_pad=None):
    """bf16 [rows, cols] -> new bf16 [cols, rows_pad] with zero-filled pad columns (rows_pad = rows rounded up to 8)."""
    _chk(src, BF16)
    rows, cols, ld = _rows_ld(src)
    rp = rows_pad or ((rows + 7) // 8 * 8)
    dst = _new((cols, rp), dtype=BF16, device=src.device)
    _lib.call('alm_transpose_bf16', src.data_ptr(), dst.data_ptr(), rows, cols, ld, rp, rp, _st())
    return dst


def pack_weight(w, dst=None, dstT=None, rows_pad=None, cols_pad=None):
    """fp32 [rows, cols] -> bf16 dst[rows_pad, >= cols_pad] and / or bf16 dstT[cols_pad, >= rows_pad], zero padded."""
    _chk(w, F32)
    rows, cols, ld = _rows_ld(w)
    rp, cp = rows_pad or rows, cols_pad or cols
    _lib.call('alm_pack_weight', w.data_ptr(), rows, cols, ld, _p(dst), dst.stride(0) if dst is not None else 0, rp, cp,
              _p(dstT), dstT.stride(0) if dstT is not None else 0, _st())


def pack_weights_multi(jobs):
    """jobs: list of (w fp32 [rows, cols] view, dst | None, dstT | None, rows_pad, cols_pad): any number of weights, 40 per launch (8 on the narrow fallback kernels)."""
    arr = (_lib.AlmPackJob * len(jobs))()
    for i, (w, dst, dstT, rp, cp) in enumerate(jobs):
        _chk(w, F32)
        rows, cols, ld = _rows_ld(w)
        arr[i] = _lib.AlmPackJob(w.data_ptr(), rows, cols, ld, _p(dst), dst.stride(0) if dst is not None else 0, rp, cp,
                                 _p(dstT), dstT.stride(0) if dstT is not None else 0)
    _lib.call('alm_pack_weights_multi', ctypes.cast(arr, ctypes.c_void_p), len(jobs), _st())


# ------------------------------------------------------------------------------------------------ LayerNorm / GEGLU

def layernorm_fwd(x, gamma, *, want_copy=False, out_f32=False, y_out=None, xc_out=None):
    """x [rows, D] fp32|bf16 -> (y bf16 (fp32 with out_f32: the final LayerNorm feeding the logit heads), xcopy bf16|None, mean, rstd)."""
    _chk(x)
    rows, D, ld = _rows_ld(x)
    y = _new((rows, D), dtype=F32 if out_f32 else BF16, device=x.device) if y_out is None else y_out
    xc = (_new((rows, D), dtype=BF16, device=x.device) if xc_out is None else xc_out) if want_copy else None
    assert y.shape == (rows, D) and y.is_contiguous() and (xc is None or (xc.shape == (rows, D) and xc.is_contiguous()))
    mean = _new(rows, dtype=F32, device=x.device)
    rstd = _new(rows, dtype=F32, device=x.device)
    _lib.call('alm_layernorm_fwd', x.data_ptr(), int(x.dtype == BF16), ld, gamma.data_ptr(), y.data_ptr(), int(out_f32), D, _p(xc), D, mean.data_ptr(),
              rstd.data_ptr(), rows, D, _st())
    return y, xc, mean, rstd


def colsum(inp, out=None, scale=1.0, accumulate=False):
    _chk(inp)
    rows, cols, ld = _rows_ld(inp)
    if out is None:
        out = _new(cols, dtype=F32, device=inp.device)
    chunks = _lib.query('alm_colsum_chunks', rows)
    ws = _new((chunks, cols), dtype=F32, device=inp.device) if chunks > 1 else None
    _lib.call('alm_colsum', inp.data_ptr(), int(inp.dtype == BF16), ld, rows, cols, out.data_ptr(), float(scale), int(accumulate), _p(ws), _st())
    return out


def layernorm_bwd(dy, x, mean, rstd, gamma, *, extra=None, dx_dtype=F32, want_dgamma=True):
    """dy bf16 (or fp32: the gradient arriving from the logit heads) -> (dx [rows, D] dx_dtype, dgamma [D] fp32 | None)."""
    _chk(dy), _chk(x)
    assert dy.dtype in (BF16, F32)
    rows, D, lddy = _rows_ld(dy)
    dx = _new((rows, D), dtype=dx_dtype, device=dy.device)
    part = None
    if want_dgamma:
        nblk = _lib.query('alm_ln_partial_blocks', rows)
        part = _new((nblk, D), dtype=F32, device=dy.device)
    _lib.call('alm_layernorm_bwd', dy.data_ptr(), int(dy.dtype == F32), lddy, x.data_ptr(), int(x.dtype == BF16), x.stride(0), mean.data_ptr(), rstd.data_ptr(),
              gamma.data_ptr(), _p(extra), extra.stride(0) if extra is not None else 0, dx.data_ptr(), int(dx_dtype == BF16), D, _p(part),
              rows, D, _st())
    return dx, (colsum(part) if want_dgamma else None)


def geglu_fwd(x):
    """fp32 [rows, 2 I] -> [rows, I]: x_half * gelu(gate_half) (the standalone GEGLU module)"""
    _chk(x, F32)
    rows, two_i, ld = _rows_ld(x)
    assert ld == two_i and two_i % 2 == 0
    y = _new((rows, two_i // 2), dtype=F32, device=x.device)
    _lib.call('alm_geglu_fwd', x.data_ptr(), y.data_ptr(), rows, two_i // 2, _st())
    return y


def geglu_bwd(dy, x):
    _chk(dy, F32), _chk(x, F32)
    rows, two_i, ld = _rows_ld(x)
    assert ld == two_i and dy.shape == (rows, two_i // 2) and dy.is_contiguous()
    dx = _new_like(x)
    _lib.call('alm_geglu_bwd', dy.data_ptr(), x.data_ptr(), dx.data_ptr(), rows, two_i // 2, _st())
    return dx


def geglu_ln_fwd(u, gamma, inner, inner_pad, out=None):
    """u bf16 [rows, 2 * inner_pad] (x | gate halves) -> (hn bf16 [rows, inner_pad] (written into `out` when given), mean, rstd)."""
    _chk(u, BF16)
    rows, _, ldu = _rows_ld(u)
    if out is None:
        out = _new((rows, inner_pad), dtype=BF16, device=u.device)
    assert out.shape == (rows, inner_pad) and out.dtype == BF16 and out.stride(1) == 1 and out.stride(0) == inner_pad
    mean = _new(rows, dtype=F32, device=u.device)
    rstd = _new(rows, dtype=F32, device=u.device)
    _lib.call('alm_geglu_ln_fwd', u.data_ptr(), ldu, inner_pad, gamma.data_ptr(), out.data_ptr(), inner_pad, mean.data_ptr(), rstd.data_ptr(),
              rows, inner, inner_pad, _st())
    return out, mean, rstd


def geglu_ln_bwd(dhn, u, gamma, mean, rstd, inner, inner_pad, du_out=None):
    """-> (du bf16 [rows, 2 * inner_pad] (written into `du_out` when given: same shape and row stride as u), dgamma [inner])."""
    rows, _, ldu = _rows_ld(u)
    du = _new_like(u) if du_out is None else du_out
    assert du.shape == u.shape and du.stride(0) == ldu and du.stride(1) == 1 and du.dtype == BF16
    nblk = _lib.query('alm_geglu_partial_blocks', rows)
    part = _new((nblk, inner), dtype=F32, device=u.device)
    _lib.call('alm_geglu_ln_bwd', dhn.data_ptr(), dhn.stride(0), u.data_ptr(), ldu, inner_pad, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              du.data_ptr(), part.data_ptr(), rows, inner, inner_pad, _st())
    return du, colsum(part)


# ------------------------------------------------------------------------------------------------ attention

def _bias_args(bias, N, H):
    """bias: object with tbl fp32 [H, LT] and int32 [N] qkey4 / kkey4 / qattr / kattr (relpos.AttnBias)."""
    tbl = _chk(bias.tbl, F32)
    assert tbl.dim() == 2 and tbl.shape[0] == H and tbl.is_contiguous(), tbl.shape
    for t in (bias.qkey4, bias.kkey4, bias.qattr, bias.kattr):
        _chk(t, torch.int32)
        assert t.shape == (N,) and t.is_contiguous(), (t.shape, N)
    return (tbl.data_ptr(), tbl.shape[1], bias.qkey4.data_ptr(), bias.kkey4.data_ptr(), bias.qattr.data_ptr(), bias.kattr.data_ptr())


def attn_bias_part(B, N, H, LT, device):
    """zeroed per-workgroup partial tables the biased attention backward accumulates the table gradient into"""
    return _new_zeros((_lib.query('alm_attn_bias_part_rows', B, N, H), LT), dtype=F32, device=device)


def attn_bias_grad_reduce(part, B, N, H, dim_head=64):
    LT = part.shape[1]
    dtbl = _new((H, LT), dtype=F32, device=part.device)
    _lib.call('alm_attn_bias_grad_reduce', part.data_ptr(), dtbl.data_ptr(), B, N, H, LT, float(dim_head) ** -0.5, _st())
    return dtbl


def mqa_attn_fwd(q, k, v, mask, B, N, H, dim_head=64, bias=None, dropout_p=0., seed=0, o=None, seed_dev=None):
    """q bf16 [B*N, H*dh]; k, v bf16 [B*N, dh] views (row stride arbitrary); mask uint8 [B, N] | None -> (o, lse).
    bias: structured score bias (see alm_mqa_attn_bias_fwd) or None.  dropout_p > 0: attention dropout with the mask stream `seed` (the
    backward must get the same pair); seed_dev (int64 [1] device tensor | None): the stream is seed + seed_dev[0], read when the kernel runs."""
    _chk(q, BF16), _chk(k, BF16), _chk(v, BF16)
    if o is None:
        o = _new((B * N, H * dim_head), dtype=BF16, device=q.device)
    assert o.shape == (B * N, H * dim_head) and o.dtype == BF16 and o.stride(1) == 1
    lse = _new((B, H, N), dtype=F32, device=q.device)
    if bias is not None:
        _lib.call('alm_mqa_attn_bias_fwd', q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), _p(mask), o.data_ptr(),
                  o.stride(0), lse.data_ptr(), B, N, H, dim_head, float(dim_head) ** -0.5, *_bias_args(bias, N, H), float(dropout_p), int(seed), _p(seed_dev), _st())
        return o, lse
    _lib.call('alm_mqa_attn_fwd', q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), _p(mask), o.data_ptr(),
              o.stride(0), lse.data_ptr(), B, N, H, dim_head, float(dim_head) ** -0.5, float(dropout_p), int(seed), _p(seed_dev), _st())
    return o, lse


def mqa_attn_bwd(q, k, v, mask, o, lse, dout, B, N, H, dim_head=64, bias=None, dtbl_part=None, dropout_p=0., seed=0, dq_out=None, seed_dev=None):
    """-> (dq bf16 [B*N, H*dh], dkv fp32 [HG, B*N, 2*dh] = per-head-group partials of (dk | dv); kv_grad_pack sums them).
    With `bias`, the table gradient is accumulated into dtbl_part (attn_bias_part)."""
    _chk(dout, BF16)
    dq = _new_like(q) if dq_out is None else dq_out
    assert dq.shape == q.shape and dq.dtype == BF16 and dq.stride(1) == 1
    hg = _lib.query('alm_mqa_bwd_parts', B, N, H)                  # dk / dv partial sets the dK/dV kernel writes for this shape (4 or 2 heads per workgroup)
    dkv = _new((hg, B * N, 2 * dim_head), dtype=F32, device=q.device)
    delta = _new((2, B, H, N), dtype=F32, device=q.device)
    if bias is not None:
        assert dtbl_part is not None and dtbl_part.shape[1] == bias.tbl.shape[1] and dtbl_part.is_contiguous()
        _lib.call('alm_mqa_attn_bias_bwd', q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), _p(mask),
                  o.data_ptr(), o.stride(0), lse.data_ptr(), dout.data_ptr(), dout.stride(0), dq.data_ptr(), dq.stride(0), dkv.data_ptr(),
                  dkv.data_ptr() + 4 * dim_head, dkv.stride(1), dkv.stride(0), delta.data_ptr(), B, N, H, dim_head, float(dim_head) ** -0.5,
                  *_bias_args(bias, N, H), dtbl_part.data_ptr(), float(dropout_p), int(seed), _p(seed_dev), _st())
        return dq, dkv
    _lib.call('alm_mqa_attn_bwd', q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), _p(mask), o.data_ptr(),
              o.stride(0), lse.data_ptr(), dout.data_ptr(), dout.stride(0), dq.data_ptr(), dq.stride(0), dkv.data_ptr(),
              dkv.data_ptr() + 4 * dim_head, dkv.stride(1), dkv.stride(0), delta.data_ptr(), B, N, H, dim_head, float(dim_head) ** -0.5,
              float(dropout_p), int(seed), _p(seed_dev), _st())
    return dq, dkv


def mqa_decode_attn(q, cache, kv_new, pos, mask, H, dim_head=64, bias=None, pos_dev=None):
    """One new position per sequence.  q bf16 [B, H*dh]; cache bf16 [B, Nmax, 2*dh] (k | v); kv_new bf16 [B, 2*dh] (appended at `pos` by the
    kernel); mask uint8 [B, >= pos+1] | None; bias: relpos.AttnBias whose index vectors cover position `pos` -> out bf16 [B, H*dh].
    pos_dev (int32 device scalar): the kernel reads the position from it instead (hipGraph replay)."""
    _chk(q, BF16), _chk(cache, BF16), _chk(kv_new, BF16)
    B, Nmax = cache.shape[0], cache.shape[1]
    assert cache.is_contiguous() and cache.shape[2] == 2 * dim_head and kv_new.shape == (B, 2 * dim_head) and kv_new.stride(1) == 1
    out = _new((B, H * dim_head), dtype=BF16, device=q.device)
    qk = qa = 0
    tb = (None, 0)
    vecs = (None, None, None, None)
    if bias is not None:
        tbl = _chk(bias.tbl, F32)
        assert tbl.is_contiguous() and tbl.shape[0] == H and bias.kkey4.shape[0] >= Nmax
        tb = (tbl.data_ptr(), tbl.shape[1])
        if pos_dev is None:
            qk, qa = int(bias.qkey4_host[pos]), int(bias.qattr_host[pos])
        vecs = (bias.kkey4.data_ptr(), bias.kattr.data_ptr(), bias.qkey4.data_ptr(), bias.qattr.data_ptr())
    _lib.call('alm_mqa_decode_attn', q.data_ptr(), q.stride(0), cache.data_ptr(), cache.stride(0), kv_new.data_ptr(), kv_new.stride(0), _p(mask),
              mask.stride(0) if mask is not None else 0, out.data_ptr(), out.stride(0), B, H, dim_head, int(pos), Nmax, float(dim_head) ** -0.5,
              tb[0], tb[1], qk, qa, vecs[0], vecs[1], _p(pos_dev), vecs[2] if pos_dev is not None else None,
              vecs[3] if pos_dev is not None else None, _st())
    return out


def value_residual_mix(v, v0):
    rows, dh, _ = _rows_ld(v)
    out = _new((rows, dh), dtype=BF16, device=v.device)
    _lib.call('alm_value_residual_mix', v.data_ptr(), v.stride(0), v0.data_ptr(), v0.stride(0), out.data_ptr(), dh, rows, dh, _st())
    return out


def loss_combine(sums, labels, weights, ignore_index=-1):
    """sums: G <= 4 fp32 scalars (per-group cross-entropy SUMS), labels: G int64 tensors, weights: G floats ->
    (loss fp32 [1] = sum_g w_g * sum_g / max(#(labels_g != ignore), 1), scales fp32 [G] = w_g / max(count_g, 1))."""
    G = len(sums)
    assert 1 <= G <= 4 and len(labels) == G and len(weights) == G
    dev = sums[0].device
    labels = [l if l.is_contiguous() else l.contiguous() for l in labels]
    for t, l in zip(sums, labels):
        _chk(t, F32)
        _chk(l, torch.int64)
    loss = _new(1, dtype=F32, device=dev)
    scales = _new(G, dtype=F32, device=dev)
    pad = [None] * (4 - G)
    _lib.call('alm_loss_combine', *[t.data_ptr() for t in sums], *pad, *[l.data_ptr() for l in labels], *pad, *[l.numel() for l in labels], *([0] * (4 - G)),
              *[float(w) for w in weights], *([0.0] * (4 - G)), G, int(ignore_index), loss.data_ptr(), scales.data_ptr(), _st())
    return loss, scales


def coarse_prepare(sem, coarse, pad_id, sem_eos, coarse_eos, Q, C, sem_has_eos=False):
    """sem int64 [B, ns0], coarse int64 [B, nc0] (flattened (n q)) -> (sem_labels [B, ns], coarse_labels [B, nc0+1], src_a int32 [B, N],
    keep bool [B, N]) with ns = ns0 + 1, N = ns + nc0 + 2: CoarseTransformerWrapper's training-step id bookkeeping (C ABI: alm_coarse_prepare).
    sem_has_eos: the rows of `sem` already are [ids | eos | pad ...] (unique_consecutive): ns = ns0."""
    _chk(sem, torch.int64), _chk(coarse, torch.int64)
    assert sem.dim() == 2 and coarse.dim() == 2 and sem.stride(1) == 1 and coarse.stride(1) == 1 and sem.shape[0] == coarse.shape[0]
    B, ns0 = sem.shape
    nc0 = coarse.shape[1]
    ns = ns0 + (0 if sem_has_eos else 1)
    N, dev = ns + nc0 + 2, sem.device
    sl = _new((B, ns), dtype=torch.int64, device=dev)
    cl = _new((B, nc0 + 1), dtype=torch.int64, device=dev)
    src_a = _new((B, N), dtype=torch.int32, device=dev)
    keep = _new((B, N), dtype=torch.bool, device=dev)
    _lib.call('alm_coarse_prepare', sem.data_ptr(), sem.stride(0), coarse.data_ptr(), coarse.stride(0), B, ns0, nc0, int(pad_id), int(sem_eos), int(coarse_eos),
              int(Q), int(C), sl.data_ptr(), cl.data_ptr(), src_a.data_ptr(), keep.data_ptr(), 1 if sem_has_eos else 0, _st())
    return sl, cl, src_a, keep


def semantic_prepare(sem, eos_id, num_rows, has_eos=False):
    """sem int64 [B, n0] -> (labels int64 [B, n0 + 1] = [ids | eos], src_a int32 [B, n0 + 1] = [start token | ids]): SemanticTransformerWrapper's training-step
    id bookkeeping + SemanticTransformer's embedding source codes (C ABI: alm_semantic_prepare).  has_eos: the rows already are [ids | eos | pad ...]
    (unique_consecutive): labels [B, n0] = the rows, src_a [B, n0] = [start token | rows without their last column]."""
    _chk(sem, torch.int64)
    assert sem.dim() == 2 and (sem.shape[1] == 0 or sem.stride(1) == 1)
    B, n0 = sem.shape
    W = n0 + (0 if has_eos else 1)
    labels = _new((B, W), dtype=torch.int64, device=sem.device)
    src_a = _new((B, W), dtype=torch.int32, device=sem.device)
    _lib.call('alm_semantic_prepare', sem.data_ptr(), sem.stride(0), B, n0, int(eos_id), int(num_rows), labels.data_ptr(), src_a.data_ptr(), 1 if has_eos else 0, _st())
    return labels, src_a


def unique_consecutive(ids, eos_id=None, pad=-1):
    """ids int64 [B, n] -> (out int64 [B, n + e], lengths int32 [B]): every row with its runs of equal ids collapsed, followed by `pad`; e = 1 and the rows
    are [ids | eos_id] when eos_id is given (C ABI: alm_unique_consecutive_i64; reference batch_unique_consecutive, audiolm_pytorch.py:162-164, after
    append_eos_id).  The caller reads `lengths` once and slices out[:, :max]."""
    _chk(ids, torch.int64)
    assert ids.dim() == 2 and (ids.shape[1] == 0 or ids.stride(1) == 1)
    B, n = ids.shape
    W = n + (0 if eos_id is None else 1)
    out = _new((B, W), dtype=torch.int64, device=ids.device)
    lengths = _new((B,), dtype=torch.int32, device=ids.device)
    if B:
        _lib.call('alm_unique_consecutive_i64', ids.data_ptr(), ids.stride(0), B, n, 0 if eos_id is None else 1, 0 if eos_id is None else int(eos_id), int(pad),
                  out.data_ptr(), W, lengths.data_ptr(), _st())
    return out, lengths


def fine_prepare(coarse, fine, nf, pad_id, eos_id, Qc, Qf, C):
    """coarse int64 [B, n], fine int64 [B, >= nf] (flattened (n q)) -> (src_a int32 [B, N], keep bool [B, N]), N = n + nf + 2: FineTransformer.forward's
    id bookkeeping (C ABI: alm_fine_prepare)."""
    _chk(coarse, torch.int64), _chk(fine, torch.int64)
    assert coarse.dim() == 2 and fine.dim() == 2 and coarse.stride(1) == 1 and fine.stride(1) == 1 and coarse.shape[0] == fine.shape[0] and fine.shape[1] >= nf
    B, n = coarse.shape
    N, dev = n + nf + 2, coarse.device
    src_a = _new((B, N), dtype=torch.int32, device=dev)
    keep = _new((B, N), dtype=torch.bool, device=dev)
    _lib.call('alm_fine_prepare', coarse.data_ptr(), coarse.stride(0), fine.data_ptr(), fine.stride(0), B, n, nf, int(pad_id), int(eos_id), int(Qc), int(Qf),
              int(C), src_a.data_ptr(), keep.data_ptr(), _st())
    return src_a, keep


FORGETFUL_MAX_N = 16384


def forgetful_mask_(keep, score, drop):
    """keep (bool [B, N]) &= NOT(one of the `drop` largest entries of its row of score (fp32 [B, N])); column 0 is never dropped (audiolm_pytorch.py:82-89)."""
    _chk(score, F32)
    assert keep.dtype == torch.bool and keep.dim() == 2 and score.shape == keep.shape and keep.stride(1) == 1 and score.stride(1) == 1
    B, N = keep.shape
    _lib.call('alm_forgetful_mask', score.data_ptr(), score.stride(0), keep.data_ptr(), keep.stride(0), B, N, int(drop), _st())
    return keep


def kv_grad_pack(dkv_f32, acc_v0, mode, dim_head=64, out=None):
    """dkv_f32: [rows, 2*dh] or per-head-group partials [HG, rows, 2*dh] (summed here) -> bf16 [rows, 2*dh]."""
    if dkv_f32.dim() == 2:
        dkv_f32 = dkv_f32.unsqueeze(0)
    nparts, rows = dkv_f32.shape[0], dkv_f32.shape[1]
    if out is None:
        out = _new((rows, 2 * dim_head), dtype=BF16, device=dkv_f32.device)
    assert out.shape == (rows, 2 * dim_head) and out.dtype == BF16 and out.stride(1) == 1
    _lib.call('alm_kv_grad_pack', dkv_f32.data_ptr(), dkv_f32.data_ptr() + 4 * dim_head, dkv_f32.stride(1), nparts, dkv_f32.stride(0),
              _p(acc_v0), out.data_ptr(), out.stride(0), rows, dim_head, mode, _st())
    return out


# ------------------------------------------------------------------------------------------------ position-bias table MLPs

def posmlp_in_fwd(x, W, b):
    """x fp32 [L, in]; W fp32 [C, in]; b [C] -> (pre fp32 [L, C], act bf16 [L, C] = silu(pre))."""
    _chk(x, F32), _chk(W, F32), _chk(b, F32)
    L, ind = x.shape
    C = W.shape[0]
    assert W.shape == (C, ind) and x.is_contiguous() and W.is_contiguous()
    pre = _new((L, C), dtype=F32, device=x.device)
    act = _new((L, C), dtype=BF16, device=x.device)
    _lib.call('alm_posmlp_in_fwd', x.data_ptr(), W.data_ptr(), b.data_ptr(), pre.data_ptr(), act.data_ptr(), L, ind, C, _st())
    return pre, act


def posmlp_in_bwd(dpre, x):
    """-> (dW fp32 [C, in], db [C])"""
    _chk(dpre, BF16), _chk(x, F32)
    L, C = dpre.shape
    ind = x.shape[1]
    chunks = _lib.query('alm_posmlp_in_bwd_chunks', L)
    part = _new((chunks, (1 + ind) * C), dtype=F32, device=x.device)
    _lib.call('alm_posmlp_in_bwd', dpre.data_ptr(), x.data_ptr(), part.data_ptr(), L, ind, C, _st())
    s = colsum(part)
    return s[C:].view(ind, C).t().contiguous(), s[:C]


def silu_fwd(pre):
    _chk(pre, F32)
    act = _new(pre.shape, dtype=BF16, device=pre.device)
    _lib.call('alm_silu_fwd', pre.data_ptr(), act.data_ptr(), pre.numel(), _st())
    return act


def silu_bwd(dact, pre):
    _chk(dact, F32), _chk(pre, F32)
    dpre = _new(pre.shape, dtype=BF16, device=pre.device)
    _lib.call('alm_silu_bwd', dact.data_ptr(), pre.data_ptr(), dpre.data_ptr(), pre.numel(), _st())
    return dpre


def posmlp_out_fwd(act, W, b, special, inv_scale):
    """act bf16 [L, C]; W fp32 [H, C]; b [H]; special fp32 [H] | None -> tbl fp32 [H, L + 1] (x inv_scale, slot 0 = special)."""
    _chk(act, BF16), _chk(W, F32), _chk(b, F32)
    L, C = act.shape
    H = W.shape[0]
    tbl = _new((H, L + 1), dtype=F32, device=act.device)
    _lib.call('alm_posmlp_out_fwd', act.data_ptr(), W.data_ptr(), b.data_ptr(), _p(special), tbl.data_ptr(), L, C, H, float(inv_scale), _st())
    return tbl


def posmlp_out_bwd(dtbl, W, pre, inv_scale):
    """-> (g bf16 [L, Hp] = d(loss)/d(last-layer output), dpre bf16 [L, C] for the layer below, dspecial fp32 [H])."""
    _chk(dtbl, F32), _chk(W, F32), _chk(pre, F32)
    H, LT = dtbl.shape
    L, C = pre.shape
    assert LT == L + 1 and dtbl.is_contiguous()
    Hp = (H + 7) // 8 * 8
    g = _new((L, Hp), dtype=BF16, device=pre.device)
    dpre = _new((L, C), dtype=BF16, device=pre.device)
    dsp = _new(H, dtype=F32, device=pre.device)
    _lib.call('alm_posmlp_out_bwd', dtbl.data_ptr(), W.data_ptr(), pre.data_ptr(), g.data_ptr(), dpre.data_ptr(), dsp.data_ptr(), L, C, H, Hp,
              float(inv_scale), _st())
    return g, dpre, dsp


# ------------------------------------------------------------------------------------------------ hyper-connections

_HC_KEYS7 = ('gamma', 'Wa', 'sa', 'Aa', 'wb', 'sb', 'Bb')


def hc_fwd(R_in, B, S, N, D, *, y_prev=None, coef_prev=None, hc=None, ln_gamma=None, final=False, want_x=True, rin_bcast=False, r_dtype=F32,
           final_f32=False, x_out=None, xn_out=None):
    """Hyper-connection forward pass over the residual streams R_in [B, S, N, D] (C ABI: alm_hc_fwd).
      y_prev / coef_prev given : depth connection of the previous branch (R = mix(R_in) + beta * y_prev)
      hc given                 : width connection + pre-LayerNorm of the next branch on that R
      final                    : depth connection + stream sum + final LayerNorm (ln_gamma); final_f32: its output in fp32 (logit heads)
      rin_bcast                : R_in is ONE fp32 [B*N, D] tensor every stream equals (right after the stream expansion)
      r_dtype                  : storage type of the stream tensors (fp32 | bf16; arithmetic is fp32 either way)
    -> dict(R=..., x, xn, mean, rstd, coef | xs, hn, mean, rstd)."""
    _chk(R_in, F32 if rin_bcast else r_dtype)
    dev, M = R_in.device, B * N
    depth, width = y_prev is not None, hc is not None
    mode = (1 if depth else 0) | (2 if width else 0) | (4 if final else 0)
    out = {}
    R_out = _new((B, S, N, D), dtype=r_dtype, device=dev) if (depth and not final) else None
    x = xn = xn32 = mean = rstd = coef = xs = None
    if width or final:
        if final and final_f32:
            xn32 = _new((M, D), dtype=F32, device=dev)
        else:
            xn = _new((M, D), dtype=BF16, device=dev) if xn_out is None else xn_out
            assert xn.shape == (M, D) and xn.dtype == BF16 and xn.is_contiguous()
        mean = _new(M, dtype=F32, device=dev)
        rstd = _new(M, dtype=F32, device=dev)
    if width:
        x = (_new((M, D), dtype=BF16, device=dev) if x_out is None else x_out) if want_x else None
        assert x is None or (x.shape == (M, D) and x.dtype == BF16 and x.is_contiguous())
        coef = _new((M, _lib.query('alm_hc_coef_width', S)), dtype=F32, device=dev)
    if final:
        xs = _new((M, D), dtype=F32, device=dev)
    hp = [hc[k].data_ptr() for k in _HC_KEYS7] if width else [None] * 7
    _lib.call('alm_hc_fwd', R_in.data_ptr(), int(rin_bcast), int(r_dtype == BF16), _p(y_prev), y_prev.stride(0) if depth else 0, _p(coef_prev), _p(R_out),
              *hp, _p(ln_gamma), _p(x), D, _p(xn), D, _p(xn32), _p(mean), _p(rstd), _p(coef), _p(xs), mode, B, S, N, D, _st())
    out.update(R=R_out if depth else R_in, x=x, xn=xn if xn32 is None else xn32, mean=mean, rstd=rstd, coef=coef, xs=xs)
    return out


def _hc_bwd_geometry(D, dx, dxn, extra, hc, y_prev, sum_only, r_dtype):
    """What hc_bwd hands alm_hc_bwd besides the pointers -- mode, fused-LayerNorm flag, storage flag, the five row strides, which of dR / dsum is asked
    for -- built in ONE place: hc_bwd launches with it and hc_bwd_variant queries the launcher's route with it."""
    width, depth = hc is not None, y_prev is not None
    ld = lambda t: t.stride(0) if t is not None else 0
    return dict(width=width, depth=depth, mode=(2 if width else 0) | (1 if depth else 0), lnf=int(width and dxn is not None), rbf=int(r_dtype == BF16),
                lddx=ld(dx), lddxn=ld(dxn), ldex=ld(extra), ldy=ld(y_prev), lddy=D, want_dR=int(width and not sum_only), want_dsum=int(width and sum_only))


def hc_bwd(dRn, B, S, N, D, *, bcast=False, dx=None, dxn=None, extra=None, mean=None, rstd=None, ln_gamma=None, R=None, coef=None, dbeta=None,
           hc=None, y_prev=None, coef_prev=None, r_bcast=False, sum_only=False, r_dtype=F32, dsum_scale=1.0, dy_out=None, defer_grads=False):
    """Hyper-connection backward (C ABI: alm_hc_bwd).  dRn: gradient wrt the residual output of a width connection, [B, S, N, D] (r_dtype), or with
    bcast fp32 [B*N, D] shared by all streams.  hc / R / coef / dbeta given: width-connection backward -> dR + the 7 parameter gradients; the
    gradient wrt the branch input is either `dx` (fp32, LayerNorm backward already applied) or `dxn` (bf16, wrt the LayerNorm output) +
    optional `extra` (bf16, added to dx) + mean / rstd / ln_gamma: then the LayerNorm backward is fused (grads['ln'] = its weight gradient).
    y_prev / coef_prev given: depth-connection backward of the previous branch on that dR (or on dRn) -> dy (bf16), dbeta_prev.
    r_bcast: R is one fp32 [B*N, D] tensor for all streams; sum_only: return dsum fp32 [B*N, D] = sum over streams of dR instead of dR.
    r_dtype: storage type of dRn / R / dR (the non-bcast forms).  dsum_scale: factor on dsum (grad_shrink's alpha rides here).
    defer_grads: the parameter gradients are NOT finished here -- `grads` is None and `part` = (partial rows, row count, hc) goes to
    hc_param_grads_batched together with the other branches' (two launches for all of them instead of two per branch).
    -> dict(dR, dsum, grads, dy, dbeta, part)."""
    geo = _hc_bwd_geometry(D, dx, dxn, extra, hc, y_prev, sum_only, r_dtype)
    width, depth, mode, rbf = geo['width'], geo['depth'], geo['mode'], geo['rbf']
    dev, M = dRn.device, B * N
    _chk(dRn, F32 if bcast else r_dtype)
    if R is not None:
        _chk(R, F32 if r_bcast else r_dtype)
    dR = dsum = part = dy = dbo = None
    if width:
        assert (dx is None) != (dxn is None)
        if sum_only:
            dsum = _new((M, D), dtype=F32, device=dev)
        else:
            dR = _new((B, S, N, D), dtype=r_dtype, device=dev)
        rows = _lib.query('alm_hc_partial_rows', mode, geo['lnf'], rbf, S, M, D)
        P = _lib.query('alm_hc_partial_width', S, D)
        part = _new((rows, P), dtype=F32, device=dev)
    if depth:
        dy = _new((M, D), dtype=BF16, device=dev) if dy_out is None else dy_out
        assert dy.shape == (M, D) and dy.dtype == BF16 and dy.is_contiguous()
        dbo = _new((M, S), dtype=F32, device=dev)
    hp = [hc[k].data_ptr() for k in ('gamma', 'Wa', 'sa', 'wb', 'sb')] if width else [None] * 5
    _lib.call('alm_hc_bwd', dRn.data_ptr(), int(bcast), rbf, _p(dx), geo['lddx'], _p(dxn), geo['lddxn'], _p(extra), geo['ldex'], _p(mean), _p(rstd),
              _p(ln_gamma), _p(R), int(r_bcast), _p(coef), _p(dbeta), *hp, _p(dR), _p(dsum), float(dsum_scale), _p(part), _p(y_prev), geo['ldy'],
              _p(coef_prev), _p(dy), geo['lddy'], _p(dbo), mode, B, S, N, D, _st())
    grads = None
    if width and defer_grads:
        return dict(dR=dR, dsum=dsum, grads=None, dy=dy, dbeta=dbo, part=(part, rows, hc))
    if width:
        chunks = _lib.query('alm_colsum_chunks', rows)
        if chunks > 1:                                       # stage 1 of the column sums; the chunk rows are summed inside alm_hc_param_grads
            ws = _new((chunks, P), dtype=F32, device=dev)
            _lib.call('alm_colsum_partial', part.data_ptr(), P, rows, P, ws.data_ptr(), _st())
        else:
            ws = colsum(part)
        g = _new(_lib.query('alm_hc_grads_width', S, D), dtype=F32, device=dev)
        _lib.call('alm_hc_param_grads', ws.data_ptr(), chunks, hc['gamma'].data_ptr(), hc['Wa'].data_ptr(), hc['wb'].data_ptr(), g.data_ptr(), S, D, _st())
        o = 0
        grads = {}
        for name, shape in (('Wa', (D, S + 1)), ('wb', (D,)), ('gamma', (D,)), ('Aa', (S, S + 1)), ('Bb', (S,)), ('sa', ()), ('sb', ()), ('ln', (D,))):
            n = 1
            for d in shape:
                n *= d
            grads[name] = g[o:o + n].view(shape)
            o += n
    return dict(dR=dR, dsum=dsum, grads=grads, dy=dy, dbeta=dbo, part=None)


def _hc_grad_views(g, S, D):
    o, grads = 0, {}
    for name, shape in (('Wa', (D, S + 1)), ('wb', (D,)), ('gamma', (D,)), ('Aa', (S, S + 1)), ('Bb', (S,)), ('sa', ()), ('sb', ()), ('ln', (D,))):
        n = 1
        for d in shape:
            n *= d
        grads[name] = g[o:o + n].view(shape)
        o += n
    return grads


def hc_param_grads_batched(parts, S, D):
    """parts: list of hc_bwd(..., defer_grads=True)['part'] = (partial rows, row count, hc) -> list of gradient dicts (keys as hc_bwd's `grads`), finished
    in two launches per 16 branches (C ABI: alm_hc_param_grads_batched)."""
    out = []
    for i0 in range(0, len(parts), 16):
        grp = parts[i0:i0 + 16]
        nb, dev = len(grp), grp[0][0].device
        P, GW = _lib.query('alm_hc_partial_width', S, D), _lib.query('alm_hc_grads_width', S, D)
        g = _new((nb, GW), dtype=F32, device=dev)
        ws = _new((nb, 16, P), dtype=F32, device=dev)
        arr_p = (ctypes.c_void_p * nb)(*[t[0].data_ptr() for t in grp])
        arr_r = (ctypes.c_int * nb)(*[int(t[1]) for t in grp])
        arr_g = (ctypes.c_void_p * nb)(*[t[2]['gamma'].data_ptr() for t in grp])
        arr_wa = (ctypes.c_void_p * nb)(*[t[2]['Wa'].data_ptr() for t in grp])
        arr_wb = (ctypes.c_void_p * nb)(*[t[2]['wb'].data_ptr() for t in grp])
        arr_o = (ctypes.c_void_p * nb)(*[g[z].data_ptr() for z in range(nb)])
        _lib.call('alm_hc_param_grads_batched', arr_p, arr_r, nb, arr_g, arr_wa, arr_wb, ws.data_ptr(), arr_o, S, D, _st())
        out += [_hc_grad_views(g[z], S, D) for z in range(nb)]
    return out


HC_BWD_VARIANTS = {-1: 'plain', 0: 'pf0', 1: 'pf1', 2: 'pf2', 3: 'gl'}


def hc_fwd_prefetch(D, *, rin_bcast=False, r_dtype=F32):
    """True when hc_fwd with these arguments launches the software-prefetching kernel (C ABI: alm_hc_fwd_prefetch -- the launcher's own choice)."""
    return bool(_lib.query('alm_hc_fwd_prefetch', int(r_dtype == BF16), int(rin_bcast), D))


def hc_bwd_variant(dRn, B, S, N, D, *, bcast=False, dx=None, dxn=None, extra=None, R=None, dbeta=None, hc=None, y_prev=None, coef_prev=None,
                   r_bcast=False, sum_only=False, r_dtype=F32, **_):
    """The kernel variant hc_bwd launches for the same keyword arguments: one of HC_BWD_VARIANTS' names (C ABI: alm_hc_bwd_variant -- the launcher's
    own choice, asked with the launch geometry hc_bwd itself uses; keywords that do not bear on the route are accepted and ignored)."""
    geo = _hc_bwd_geometry(D, dx, dxn, extra, hc, y_prev, sum_only, r_dtype)
    # the launcher's al16: every row the LDS-DMA kernel reads starts on a 16-byte boundary (NULL counts as aligned), coef_prev and dbeta are given
    al16 = all(t is None or t.data_ptr() % 16 == 0 for t in (dRn, R, dxn, extra, y_prev)) and (geo['lddxn'] | geo['ldex'] | geo['ldy']) % 8 == 0
    al16 = al16 and coef_prev is not None and dbeta is not None
    ld_max = max(geo['lddx'], geo['lddxn'], geo['ldex'], geo['ldy'], geo['lddy'])
    v = _lib.query('alm_hc_bwd_variant', geo['mode'], geo['lnf'], geo['rbf'], S, B, N, D, int(bcast), int(r_bcast), geo['want_dR'], geo['want_dsum'],
                   ld_max, int(al16))
    return HC_BWD_VARIANTS[v]


# un-fused single-connection forms (kernel tests; the product path uses the fused modes)
def hc_width_fwd(R, hc, ln_gamma, B, S, N, D, want_x=True):
    r = hc_fwd(R, B, S, N, D, hc=hc, ln_gamma=ln_gamma, want_x=want_x, r_dtype=R.dtype)
    return r['x'], r['xn'], r['mean'], r['rstd'], r['coef']


def hc_depth_fwd(R, y, coef, B, S, N, D):
    return hc_fwd(R, B, S, N, D, y_prev=y, coef_prev=coef, r_dtype=R.dtype)['R']


def hc_depth_bwd(dRn, y, coef, B, S, N, D, bcast=False):
    r = hc_bwd(dRn, B, S, N, D, bcast=bcast, y_prev=y, coef_prev=coef, r_dtype=F32 if bcast else dRn.dtype)
    return r['dy'], r['dbeta']


def hc_width_bwd(dRn, dx, R, coef, dbeta, hc, B, S, N, D):
    r = hc_bwd(dRn, B, S, N, D, dx=dx, R=R, coef=coef, dbeta=dbeta, hc=hc, r_dtype=R.dtype)
    return r['dR'], r['grads']


def streams_expand(x, B, S):
    _chk(x, F32)
    nd = x.numel() // B
    R = _new((B, S) + tuple(x.shape[1:]), dtype=F32, device=x.device)
    _lib.call('alm_streams_expand', x.data_ptr(), R.data_ptr(), B, S, nd, _st())
    return R


def streams_reduce(R, B, S):
    nd = R.numel() // (B * S)
    x = _new((B,) + tuple(R.shape[2:]), dtype=F32, device=R.device)
    _lib.call('alm_streams_reduce', R.data_ptr(), x.data_ptr(), B, S, nd, _st())
    return x


def residual_add(x, y):
    """fp32 x [rows, D] + bf16 y [rows, D] -> new fp32."""
    rows, D = y.shape
    out = _new((rows, D), dtype=F32, device=y.device)
    _lib.call('alm_residual_add', x.data_ptr(), y.data_ptr(), y.stride(0), out.data_ptr(), rows, D, _st())
    return out


def f32_to_bf16(a, b=None, out=None):
    rows, D = a.shape
    if out is None:
        out = _new((rows, D), dtype=BF16, device=a.device)
    assert out.shape == (rows, D) and out.dtype == BF16 and out.is_contiguous()
    _lib.call('alm_f32_to_bf16', a.data_ptr(), _p(b), out.data_ptr(), D, rows, D, _st())
    return out


def add_f32(a, b, scale=1.0):
    """(a + b) * scale, fp32"""
    out = _new_like(a)
    _lib.call('alm_add_f32', a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), float(scale), _st())
    return out


# ------------------------------------------------------------------------------------------------ token-id side

def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


_err_flags = {}


def device_error_flag(device):
    """int32 device word the id-consuming kernels raise when they meet an id outside its table (the reference's nn.Embedding would raise
    IndexError; the kernels never dereference such an id).  Poll it with check_device_errors() at a point where a sync is acceptable."""
    key = (device.type, device.index)
    if key not in _err_flags:
        with torch.inference_mode(False):       # the word outlives the call: created under inference_mode (a text= encode, generate()) it could not be zeroed later
            _err_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _err_flags[key]


def check_device_errors(device=None):
    """Raises IndexError if any embedding lookup since the last check saw an out-of-range token id (synchronises)."""
    for key, flag in list(_err_flags.items()):
        if device is not None and (device.type, device.index) != key:
            continue
        if int(flag.item()) != 0:
            flag.zero_()
            _err_poll.pop(key, None)
            raise IndexError('token id out of range of its embedding table (audiolm_pytorch_amd embed_assemble): the offending positions were '
                             'embedded as zero vectors')


_err_poll = {}
CHECK_IDS = __import__('os').environ.get('ALM_CHECK_IDS', '1') != '0'


def poll_device_errors(device):
    """Non-blocking form of check_device_errors(), called by every embedding lookup (ALM_CHECK_IDS=0 turns it off): the error word is copied to
    pinned host memory asynchronously and the copy issued by an EARLIER call is examined once it has landed -- an out-of-range token id therefore
    raises IndexError (what the reference's nn.Embedding does at once) one or two lookups late, without a host-device synchronisation anywhere.
    Skipped while a hipGraph is being captured (events cannot be queried there)."""
    if not CHECK_IDS or device.type != 'cuda' or torch.cuda.is_current_stream_capturing():
        return
    key = (device.type, device.index)
    flag = _err_flags.get(key)
    if flag is None:
        return
    st = _err_poll.get(key)
    if st is None:
        with torch.inference_mode(False):       # as device_error_flag: the pinned copy is written by later calls outside inference_mode
            st = _err_poll[key] = [torch.zeros(1, dtype=torch.int32).pin_memory(), None]
    host, ev = st
    if ev is not None:
        if not ev.query():
            return                                            # the previous copy is still in flight: look again at the next lookup
        st[1] = None
        if int(host[0]) != 0:
            flag.zero_()
            host.zero_()
            raise IndexError('token id out of range of its embedding table (audiolm_pytorch_amd embed_assemble, an earlier step): the offending '
                             'positions were embedded as zero vectors')
    host.copy_(flag, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    st[1] = ev


def _table_rows(tables):
    return (ctypes.c_int * len(tables))(*[t.shape[0] for t in tables])


def embed_assemble(tables, src_a, src_b, rows, D):
    """tables: fp32 [rows_t, D] each.  Ids outside a table never touch memory: zero vector + device error flag (see device_error_flag)."""
    out = _new((rows, D), dtype=F32, device=src_a.device)
    arr = _ptr_array(tables)
    poll_device_errors(src_a.device)
    _lib.call('alm_embed_assemble', ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(_table_rows(tables), ctypes.c_void_p), len(tables), src_a.data_ptr(),
              src_b.data_ptr(), out.data_ptr(), rows, D, device_error_flag(src_a.device).data_ptr(), _st())
    return out


def embed_scatter_add(grad_tables, src_a, src_b, dout, alpha, rows, D):
    arr = _ptr_array(grad_tables)
    _lib.call('alm_embed_scatter_add', ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(_table_rows(grad_tables), ctypes.c_void_p), len(grad_tables),
              src_a.data_ptr(), src_b.data_ptr(), dout.data_ptr(), float(alpha), rows, D, _st())


# fp32 elements of chunk partials the owned scatter may allocate per backward (default 2^28 = 1 GiB); above it the atomic kernel runs (ALM_EMBED_SCATTER_WS_CAP)
EMBED_SCATTER_WS_CAP = int(os.environ.get('ALM_EMBED_SCATTER_WS_CAP', str(1 << 28)))


def embed_scatter_owned(grad_tables, src_a, src_b, dout, alpha, rows, D):
    """deterministic form of embed_scatter_add (one owner per destination row, fixed summation order, no atomics): WRITES every row of every table --
    `grad_tables` may be uninitialised memory (alm_embed_scatter_owned).  -> True; False when the size is outside its range and the atomic kernel ran instead"""
    arr, tr = _ptr_array(grad_tables), _table_rows(grad_tables)
    nws = _lib.query('alm_embed_scatter_ws_floats', ctypes.cast(tr, ctypes.c_void_p), len(grad_tables), rows, D)
    if nws < 0 or nws > EMBED_SCATTER_WS_CAP:
        # outside the owned kernel's range (rows >= 2^28, or a chunk-partial workspace that grows with B * N beyond the cap: ~0.5 GB at 128 k tokens):
        # the atomic kernel takes over on zeroed tables -- same sums, arrival-order rounding (the caller is told through the return value)
        for g in grad_tables:
            g.zero_()
        embed_scatter_add(grad_tables, src_a, src_b, dout, alpha, rows, D)
        return False
    ws = _new(max(nws, 1), dtype=F32, device=dout.device)
    _lib.call('alm_embed_scatter_owned', ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(tr, ctypes.c_void_p), len(grad_tables),
              src_a.data_ptr(), src_b.data_ptr(), dout.data_ptr(), float(alpha), rows, D, ws.data_ptr(), _st())
    return True


def gather_split(inp, idx=None, rows_out=None, out=None):
    """fp32 inp [rows_in, D] (row stride arbitrary) -> (hi, lo) bf16 [rows_out, D] with hi + lo ~= inp[idx] to ~16 mantissa bits: the split-bf16
    operands of the logit heads.  idx int32 [rows_out] (-1 = zero row) or None (identity; rows past rows_in are zero = row padding).
    out = (hi, lo): bf16 [rows_out, D] views of ONE row stride (column blocks of a wider buffer: the K-concatenated head operands)."""
    _chk(inp, F32)
    rows_in, D, ld = _rows_ld(inp)
    if idx is not None:
        rows_out = idx.numel()
    elif rows_out is None:
        rows_out = rows_in
    if out is None:
        hi = _new((rows_out, D), dtype=BF16, device=inp.device)
        lo = _new((rows_out, D), dtype=BF16, device=inp.device)
    else:
        hi, lo = out
        assert hi.shape == lo.shape == (rows_out, D) and hi.dtype == lo.dtype == BF16 and hi.stride(1) == lo.stride(1) == 1 and hi.stride(0) == lo.stride(0)
    _lib.call('alm_gather_split_bf16', inp.data_ptr(), ld, rows_in, _p(idx), hi.data_ptr(), lo.data_ptr(), hi.stride(0), rows_out, D, _st())
    return hi, lo


def gather_rows(inp, idx, out=None):
    rows = idx.numel()
    D = inp.shape[1]
    if out is None:
        out = _new((rows, D), dtype=BF16, device=inp.device)
    _lib.call('alm_gather_rows_bf16', inp.data_ptr(), inp.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), rows, D, _st())
    return out


def scatter_rows(inp, idx, out):
    rows = idx.numel()
    _lib.call('alm_scatter_rows_bf16', inp.data_ptr(), inp.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), rows, inp.shape[1], _st())
    return out


def cross_entropy_fwd(logits, labels, C, ignore_index=-1):
    """logits fp32 [rows, >= C]; labels int64 [rows] -> (loss_rows fp32, lse fp32)."""
    _chk(logits, F32), _chk(labels, torch.int64)
    rows = labels.numel()
    loss = _new(rows, dtype=F32, device=logits.device)
    lse = _new(rows, dtype=F32, device=logits.device)
    _lib.call('alm_cross_entropy_fwd', logits.data_ptr(), logits.stride(0), labels.data_ptr(), loss.data_ptr(), lse.data_ptr(), rows, C, ignore_index, _st())
    return loss, lse


def cross_entropy_bwd(logits, labels, lse, gscale, C, Cpad, ignore_index=-1):
    rows = labels.numel()
    d = _new((rows, Cpad), dtype=BF16, device=logits.device)
    _lib.call('alm_cross_entropy_bwd', logits.data_ptr(), logits.stride(0), labels.data_ptr(), lse.data_ptr(), gscale.data_ptr(), d.data_ptr(), Cpad,
              rows, C, Cpad, ignore_index, _st())
    return d


def reduce_sum(x, scale=1.0):
    out = _new((), dtype=F32, device=x.device)
    _lib.call('alm_reduce_sum', x.data_ptr(), x.numel(), out.data_ptr(), float(scale), _st())
    return out


# ------------------------------------------------------------------------------------------------ SoundStream tokenize path

def conv1d_pack(w):
    """nn.Conv1d weight fp32 [Cout, Cin, k] -> packed [k][Cin_pad][Cout_pad] fp32 (once per weight update)."""
    _chk(w, F32)
    Cout, Cin, ks = w.shape
    wp = _new(_lib.query('alm_conv1d_packed_floats', Cout, Cin, ks), dtype=F32, device=w.device)
    _lib.call('alm_conv1d_pack', w.contiguous().data_ptr(), wp.data_ptr(), Cout, Cin, ks, _st())
    return wp


def conv1d_causal(x, wp, bias, Cout, ksize, *, stride=1, dilation=1, elu=False, residual=None, zero_pad=False):
    """x fp32 [B, Cin, T] -> fp32 [B, Cout, T // stride]: CausalConv1d (reflect left pad; zero_pad: zeros) + bias (+ ELU) (+ residual)."""
    _chk(x, F32)
    B, Cin, T = x.shape
    assert x.is_contiguous()
    Tout = (T - stride) // stride + 1
    out = _new((B, Cout, Tout), dtype=F32, device=x.device)
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous()
    _lib.call('alm_conv1d_causal', x.data_ptr(), wp.data_ptr(), bias.data_ptr(), _p(residual), out.data_ptr(), B, Cin, Cout, T, ksize, stride,
              dilation, int(elu), int(zero_pad), _st())
    return out


def resunit_supported(C):
    return C % 32 == 0 and C <= 256


def resunit_causal(x, w7p, b7, w1p, b1, ksize, dilation):
    """x fp32 [B, C, T] -> x + ELU(conv_k1(ELU(conv_k,dilation(x)))) in one launch (alm_resunit_causal; C % 32 == 0, C <= 256)"""
    _chk(x, F32)
    B, C, T = x.shape
    assert x.is_contiguous()
    out = _new_like(x)
    _lib.call('alm_resunit_causal', x.data_ptr(), w7p.data_ptr(), b7.data_ptr(), w1p.data_ptr(), b1.data_ptr(), out.data_ptr(), B, C, T, ksize, dilation, _st())
    return out


def phase_interleave(y, Cout, s):
    """y fp32 [B, s * Cout, n] (phase-major channels) -> [B, Cout, n * s]: out[b, co, q * s + r] = y[b, r * Cout + co, q]."""
    _chk(y, F32)
    B, SC, n = y.shape
    assert SC == s * Cout and y.is_contiguous()
    out = _new((B, Cout, n * s), dtype=F32, device=y.device)
    _lib.call('alm_phase_interleave', y.data_ptr(), out.data_ptr(), B, Cout, s, n, _st())
    return out


def rvq_decode(idx, E, out):
    """idx int64 [T, Q] (row stride arbitrary, -1 = no code), E fp32 [Q, C, d] -> out fp32 [T, d] view (row stride arbitrary): summed code vectors."""
    _chk(E, F32), _chk(out, F32)
    assert idx.dtype == torch.int64 and idx.stride(1) == 1 and out.stride(1) == 1 and E.is_contiguous()
    T, Q = idx.shape
    _lib.call('alm_rvq_decode', idx.data_ptr(), idx.stride(0), E.data_ptr(), out.data_ptr(), out.stride(0), T, E.shape[2], E.shape[1], Q, _st())
    return out


def rvq_pack(E):
    """codebooks fp32 [Q, C, d] -> (Et [Q, dpad, Cpad] MFMA-ordered image, e2 [Q, Cpad])."""
    _chk(E, F32)
    Q, C, d = E.shape
    CP = _lib.query('alm_rvq_padded_codes', C)
    Et = _new((Q, _lib.query('alm_rvq_padded_dim', d), CP), dtype=F32, device=E.device)
    e2 = _new((Q, CP), dtype=F32, device=E.device)
    _lib.call('alm_rvq_pack', E.contiguous().data_ptr(), Et.data_ptr(), e2.data_ptr(), Q, C, d, _st())
    return Et, e2


def rvq_encode(x, E, Et, e2, idx_out=None, quant_out=None):
    """x fp32 [T, d] (row stride arbitrary) against codebooks E [Q, C, d] -> int64 indices [T, Q] (written into idx_out view if given)."""
    _chk(x, F32)
    T, d = x.shape
    Q, C, _ = E.shape
    assert x.stride(1) == 1
    if idx_out is None:
        idx_out = _new((T, Q), dtype=torch.int64, device=x.device)
    assert idx_out.shape == (T, Q) and idx_out.stride(1) == 1
    _lib.call('alm_rvq_encode', x.data_ptr(), x.stride(0), E.data_ptr(), Et.data_ptr(), e2.data_ptr(), idx_out.data_ptr(), idx_out.stride(0),
              _p(quant_out), quant_out.stride(0) if quant_out is not None else 0, T, d, C, Q, _st())
    return idx_out


# ---- train-mode residual VQ (csrc/rvq_train.hip): fp32, no atomics, bitwise reproducible

def _idx_col(idx):
    """(pointer, row stride) of an int64 index column [M] (any stride) or of the first column of an [M, Q] array"""
    _chk(idx, torch.int64)
    assert idx.ndim == 1 or idx.stride(1) == 1
    return idx.data_ptr(), idx.stride(0)


def rvq_code_stats_chunk():
    """rows per chunk of a code's row list in alm_rvq_code_stats (a code with more rows is summed as several partials, added in chunk order)"""
    return _lib.query('alm_rvq_code_stats_chunk')


def rvq_code_stats(r, idx, C, n_out=None, s_out=None):
    """r fp32 [M, d] (row stride arbitrary), idx int64 [M] (any stride; -1 = skip) -> (n [C] rows per code as floats, s [C, d] their sums)"""
    _chk(r, F32)
    M, d = r.shape
    assert r.stride(1) == 1 and idx.shape == (M,)
    nws = _lib.query('alm_rvq_code_stats_ws_floats', M, d, C)
    if nws < 0:
        raise _lib.AlmError(f'alm_rvq_code_stats: workspace for M = {M}, d = {d}, C = {C} does not fit an int')
    ws = _new((max(nws, 1),), dtype=F32, device=r.device)
    n = _new((C,), dtype=F32, device=r.device) if n_out is None else n_out
    s = _new((C, d), dtype=F32, device=r.device) if s_out is None else s_out
    assert n.is_contiguous() and s.is_contiguous() and n.shape == (C,) and s.shape == (C, d)
    ip, ldi = _idx_col(idx)
    _lib.call('alm_rvq_code_stats', r.data_ptr(), r.stride(0), ip, ldi, n.data_ptr(), s.data_ptr(), ws.data_ptr(), nws, M, d, C, _st())
    return n, s


def rvq_train_quantize(resid, idx, E, out, loss, loss_scale, rotation):
    """one layer in place: resid [M, d] -= y, out [M, d] view += y, loss (one float) = loss_scale * sum |E[idx] - resid|^2  (alm_rvq_train_quantize)"""
    _chk(resid, F32), _chk(E, F32), _chk(out, F32), _chk(loss, F32)
    M, d = resid.shape
    C = E.shape[0]
    assert resid.stride(1) == 1 and out.stride(1) == 1 and out.shape == (M, d) and E.is_contiguous() and E.shape == (C, d) and idx.shape == (M,)
    part = _new((max(_lib.query('alm_rvq_train_quantize_blocks', M), 1),), dtype=F32, device=resid.device)
    ip, ldi = _idx_col(idx)
    _lib.call('alm_rvq_train_quantize', resid.data_ptr(), resid.stride(0), ip, ldi, E.data_ptr(), out.data_ptr(), out.stride(0), loss.data_ptr(), part.data_ptr(),
              float(loss_scale), int(rotation), M, d, C, _st())


def rvq_ema_update(cluster_size, embed_avg, embed, n, s, decay, eps, threshold, dead):
    """EMA + Laplace smoothing + embed rewrite of one layer; dead int32 [1 + C] <- (number of codes below `threshold`, then those codes ascending)"""
    for t in (cluster_size, embed_avg, embed, n, s):
        _chk(t, F32)
        assert t.is_contiguous()
    C, d = embed.shape[-2:]
    assert cluster_size.numel() == C and embed_avg.numel() == C * d and n.numel() == C and s.numel() == C * d
    assert dead.dtype == torch.int32 and dead.is_contiguous() and dead.numel() >= 1 + C
    total = _new((1,), dtype=F32, device=embed.device)
    _lib.call('alm_rvq_ema_update', cluster_size.data_ptr(), embed_avg.data_ptr(), embed.data_ptr(), n.data_ptr(), s.data_ptr(), float(decay), float(eps),
              float(threshold), dead.data_ptr(), total.data_ptr(), C, d, _st())


def rvq_expire(dead_codes, count, rows, x, idx, E, q, rotation, threshold, cluster_size, embed_avg, embed):
    """codes dead_codes[:count] (int32, device) <- the layer-q residual of the rows `rows` (int64 [count], device) of x, recomputed from idx [M, Q] and E [Q, C, d]"""
    _chk(x, F32), _chk(E, F32), _chk(rows, torch.int64)
    M, d = x.shape
    C = E.shape[1]
    assert x.stride(1) == 1 and E.is_contiguous() and rows.is_contiguous() and rows.numel() == count and idx.stride(1) == 1 and idx.shape[0] == M
    assert dead_codes.dtype == torch.int32 and dead_codes.is_contiguous() and dead_codes.numel() >= count
    _lib.call('alm_rvq_expire', dead_codes.data_ptr(), count, rows.data_ptr(), x.data_ptr(), x.stride(0), idx.data_ptr(), idx.stride(0), E.data_ptr(), q,
              int(rotation), float(threshold), cluster_size.data_ptr(), embed_avg.data_ptr(), embed.data_ptr(), M, d, C, _st())


def rvq_kmeans_update(means, n, s, embed=None, embed_avg=None, cluster_size=None):
    """means [C, d] = n == 0 ? means : s / max(n, 1) in place; with `embed` also embed = means, embed_avg = means * n, cluster_size = n"""
    _chk(means, F32)
    C, d = means.shape
    assert means.is_contiguous() and n.is_contiguous() and s.is_contiguous()
    _lib.call('alm_rvq_kmeans_update', means.data_ptr(), n.data_ptr(), s.data_ptr(), _p(embed), _p(embed_avg), _p(cluster_size), C, d, _st())


def rvq_train_bwd(x, idx, E, g_out, coef, dx, rotation):
    """dx [M, d] view <- the input gradient of the train-mode residual VQ of one group (alm_rvq_train_bwd); g_out [M, d] view or None, coef [Q] or None"""
    _chk(x, F32), _chk(E, F32), _chk(dx, F32), _chk(idx, torch.int64)
    M, d = x.shape
    Q, C, _ = E.shape
    assert x.stride(1) == 1 and dx.stride(1) == 1 and E.is_contiguous() and idx.shape == (M, Q) and idx.stride(1) == 1
    assert g_out is None or (g_out.dtype == F32 and g_out.stride(1) == 1 and g_out.shape == (M, d))
    assert coef is None or (coef.dtype == F32 and coef.is_contiguous() and coef.numel() == Q)
    _lib.call('alm_rvq_train_bwd', x.data_ptr(), x.stride(0), idx.data_ptr(), idx.stride(0), E.data_ptr(), _p(g_out), g_out.stride(0) if g_out is not None else 0,
              _p(coef), dx.data_ptr(), dx.stride(0), int(rotation), M, d, C, Q, _st())


def bct_to_btc(x):
    B, C, T = x.shape
    out = _new((B, T, C), dtype=F32, device=x.device)
    _lib.call('alm_bct_to_btc', x.data_ptr(), out.data_ptr(), B, C, T, _st())
    return out


# ---- backward of the codec's conv stacks (csrc/codec_bwd.hip), exact fp32, no atomics

def conv1d_pack_t(w):
    """nn.Conv1d weight fp32 [Cout, Cin, k] -> the image alm_conv1d_dgrad reads: alm_conv1d_pack of the transposed weight, [k][Cout_pad][Cin_pad]."""
    _chk(w, F32)
    return conv1d_pack(w.transpose(0, 1).contiguous())


def conv1d_dgrad(g, y, wt, Cin, Tin, ksize, *, stride=1, dilation=1, zero_pad=False, residual=None):
    """g fp32 [B, Cout, Tout] (= dL/dout; times ELU'(y) when the saved post-ELU output y is given) -> dL/dx fp32 [B, Cin, Tin] of conv1d_causal,
    reflect fold included (+ residual [B, Cin, Tin]).  wt: conv1d_pack_t image."""
    _chk(g, F32), _chk(wt, F32)
    B, Cout, Tout = g.shape
    assert g.is_contiguous() and Tout == (Tin - stride) // stride + 1
    if y is not None:
        _chk(y, F32)
        assert y.shape == g.shape and y.is_contiguous()
    dx = _new((B, Cin, Tin), dtype=F32, device=g.device)
    if residual is not None:
        _chk(residual, F32)
        assert residual.shape == dx.shape and residual.is_contiguous()
    _lib.call('alm_conv1d_dgrad', g.data_ptr(), _p(y), wt.data_ptr(), _p(residual), dx.data_ptr(), B, Cin, Cout, Tin, ksize, stride, dilation,
              int(zero_pad), _st())
    return dx


def conv1d_wgrad(g, y, x, ksize, *, stride=1, dilation=1, zero_pad=False):
    """g fp32 [B, Cout, Tout] (times ELU'(y) when y is given), x fp32 [B, Cin, Tin] -> (dW fp32 [Cout, Cin, k], db fp32 [Cout]) of conv1d_causal;
    per-chunk partials in a workspace of alm_conv1d_wgrad_ws_floats floats, summed in chunk order."""
    _chk(g, F32), _chk(x, F32)
    B, Cout, Tout = g.shape
    _, Cin, Tin = x.shape
    assert g.is_contiguous() and x.is_contiguous() and x.shape[0] == B and Tout == (Tin - stride) // stride + 1
    if y is not None:
        _chk(y, F32)
        assert y.shape == g.shape and y.is_contiguous()
    n = _lib.query('alm_conv1d_wgrad_ws_floats', B, Cin, Cout, Tout, ksize)
    if n < 0:
        raise _lib.AlmError('conv1d_wgrad: the partial-sum workspace exceeds 2^31 floats')
    ws = _new((n,), dtype=F32, device=g.device)
    dw = _new((Cout, Cin, ksize), dtype=F32, device=g.device)
    db = _new((Cout,), dtype=F32, device=g.device)
    _lib.call('alm_conv1d_wgrad', g.data_ptr(), _p(y), x.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), n, B, Cin, Cout, Tin, ksize, stride,
              dilation, int(zero_pad), _st())
    return dw, db


def phase_deinterleave(g, Cout, s):
    """g fp32 [B, Cout, n * s] -> [B, s * Cout, n] (phase-major channels): the adjoint of phase_interleave."""
    _chk(g, F32)
    B, C, Ts = g.shape
    assert C == Cout and Ts % s == 0 and g.is_contiguous()
    n = Ts // s
    y = _new((B, s * Cout, n), dtype=F32, device=g.device)
    _lib.call('alm_phase_deinterleave', g.data_ptr(), y.data_ptr(), B, Cout, s, n, _st())
    return y


def _rows(x):
    """fp32 [R, L] with unit element stride -> (tensor, row stride); copies only when the rows are not evenly strided"""
    if x.stride(-1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def resample_sinc(x, table, o, n, W):
    """x fp32 [R, L] -> fp32 [R, ceil(n L / o)]: the windowed-sinc polyphase resampler (alm_resample_sinc; table fp32 [n, 2 W + o])."""
    _chk(x, F32)
    _chk(table, F32)
    assert x.dim() == 2 and table.is_contiguous() and table.shape == (n, 2 * W + o)
    R, L = x.shape
    x, ld = _rows(x)
    Lout = (n * L + o - 1) // o
    out = _new((R, Lout), dtype=F32, device=x.device)
    _lib.call('alm_resample_sinc', x.data_ptr(), ld, out.data_ptr(), Lout, table.data_ptr(), 2 * W + o, R, L, Lout, o, n, W, _st())
    return out


def resample_sinc_bwd(dy, table, L, o, n, W):
    """dy fp32 [R, ceil(n L / o)] -> dx fp32 [R, L]: the adjoint of resample_sinc (alm_resample_sinc_bwd)."""
    _chk(dy, F32)
    _chk(table, F32)
    assert dy.dim() == 2 and table.is_contiguous() and table.shape == (n, 2 * W + o)
    R, Lout = dy.shape
    dy, ld = _rows(dy)
    dx = _new((R, L), dtype=F32, device=dy.device)
    _lib.call('alm_resample_sinc_bwd', dy.data_ptr(), ld, dx.data_ptr(), L, table.data_ptr(), 2 * W + o, R, L, Lout, o, n, W, _st())
    return dx


# ---- SoundStream LocalTransformer (csrc/local_attn.hip), fp32, codec layout [B, C, T]

def layernorm_bct(x, gamma, beta, eps=1e-5):
    _chk(x, F32)
    B, C, T = x.shape
    assert x.is_contiguous()
    out = _new_like(x)
    _lib.call('alm_layernorm_bct', x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B, C, T, float(eps), _st())
    return out


def geglu_bct(x):
    """x fp32 [B, 2 I, T] -> [B, I, T]: x[:, :I] * gelu(x[:, I:])"""
    _chk(x, F32)
    B, C2, T = x.shape
    assert x.is_contiguous() and C2 % 2 == 0
    out = _new((B, C2 // 2, T), dtype=F32, device=x.device)
    _lib.call('alm_geglu_bct', x.data_ptr(), out.data_ptr(), B, C2 // 2, T, _st())
    return out


def local_attn(qkv, q_scale, k_scale, cos_t, sin_t, xpos_t, gates, heads, dim_head, window, scale):
    """qkv fp32 [B, 3 H dh, T], gates fp32 [B, H, T] | None, slot tables [2 window, dh] -> [B, H dh, T]"""
    _chk(qkv, F32)
    B, C3, T = qkv.shape
    assert qkv.is_contiguous() and C3 == 3 * heads * dim_head
    for t in (cos_t, sin_t, xpos_t):
        assert t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == (2 * window, dim_head) and t.device == qkv.device
    out = _new((B, heads * dim_head, T), dtype=F32, device=qkv.device)
    _lib.call('alm_local_attn', qkv.data_ptr(), q_scale.data_ptr(), k_scale.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), xpos_t.data_ptr(), _p(gates),
              out.data_ptr(), B, heads, dim_head, T, window, float(scale), _st())
    return out


# ---- their backward (csrc/local_attn_bwd.hip), exact fp32, no atomics

def local_attn_bwd_supported(dim_head, window):
    """the geometries alm_local_attn_bwd covers, which are those of alm_local_attn: dim_head in {32, 64}, window <= 256, 4 dim_head window floats of LDS <= 160 KiB"""
    return bool(_lib.query('alm_local_attn_bwd_supported', int(dim_head), int(window)))


def local_attn_bwd(qkv, q_scale, k_scale, cos_t, sin_t, xpos_t, gates, o, do, heads, dim_head, window, scale):
    """qkv / gates / slot tables as for local_attn, o = its saved (gated) output, do = dL/do [B, H dh, T] ->
    (dqkv [B, 3 H dh, T], dgates [B, H, T], dq_scale [dh], dk_scale [dh])"""
    for t in (qkv, gates, o, do):
        _chk(t, F32)
    B, C3, T = qkv.shape
    assert qkv.is_contiguous() and C3 == 3 * heads * dim_head
    assert gates.is_contiguous() and tuple(gates.shape) == (B, heads, T)
    assert o.is_contiguous() and do.is_contiguous() and tuple(o.shape) == tuple(do.shape) == (B, heads * dim_head, T)
    for t in (cos_t, sin_t, xpos_t):
        assert t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == (2 * window, dim_head) and t.device == qkv.device
    for t in (q_scale, k_scale):
        assert t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == (dim_head,) and t.device == qkv.device
    if not local_attn_bwd_supported(dim_head, window):
        raise _lib.AlmError(f'local_attn_bwd: dim_head {dim_head} / window {window} is outside the kernel\'s envelope (dim_head 32 or 64, window <= 256, '
                            'dim_head 64 up to window 160)')
    n = _lib.query('alm_local_attn_bwd_ws_floats', B, heads, dim_head, T, window)
    if n < 0:
        raise _lib.AlmError('local_attn_bwd: the workspace exceeds 2^31 floats')
    ws = _new((n,), dtype=F32, device=qkv.device)
    dqkv = _new_like(qkv)
    dgates = _new_like(gates)
    dqs = _new((dim_head,), dtype=F32, device=qkv.device)
    dks = _new((dim_head,), dtype=F32, device=qkv.device)
    _lib.call('alm_local_attn_bwd', qkv.data_ptr(), q_scale.data_ptr(), k_scale.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), xpos_t.data_ptr(),
              gates.data_ptr(), o.data_ptr(), do.data_ptr(), dqkv.data_ptr(), dgates.data_ptr(), dqs.data_ptr(), dks.data_ptr(), ws.data_ptr(), n,
              B, heads, dim_head, T, window, float(scale), _st())
    return dqkv, dgates, dqs, dks


def layernorm_bct_bwd(dy, x, gamma, eps=1e-5, *, residual=None, need_params=True):
    """dy, x (the forward input) fp32 [B, C, T], gamma [C] -> (dx [B, C, T] (+ residual), dgamma [C] | None, dbeta [C] | None)"""
    _chk(dy, F32), _chk(x, F32), _chk(gamma, F32)
    B, C, T = x.shape
    assert x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape and gamma.is_contiguous() and tuple(gamma.shape) == (C,)
    if residual is not None:
        _chk(residual, F32)
        assert residual.shape == x.shape and residual.is_contiguous()
    n = _lib.query('alm_layernorm_bct_bwd_ws_floats', B, T)
    if n < 0:
        raise _lib.AlmError('layernorm_bct_bwd: the statistics workspace exceeds 2^31 floats')
    ws = _new((n,), dtype=F32, device=x.device)
    dx = _new_like(x)
    dgamma = _new((C,), dtype=F32, device=x.device) if need_params else None
    dbeta = _new((C,), dtype=F32, device=x.device) if need_params else None
    _lib.call('alm_layernorm_bct_bwd', dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), _p(residual), dx.data_ptr(), _p(dgamma), _p(dbeta), ws.data_ptr(),
              B, C, T, float(eps), _st())
    return dx, dgamma, dbeta


def geglu_bct_bwd(dh, u):
    """dh fp32 [B, I, T], u fp32 [B, 2 I, T] (the input of geglu_bct) -> du [B, 2 I, T]"""
    _chk(dh, F32), _chk(u, F32)
    B, C2, T = u.shape
    assert u.is_contiguous() and dh.is_contiguous() and C2 % 2 == 0 and tuple(dh.shape) == (B, C2 // 2, T)
    du = _new_like(u)
    _lib.call('alm_geglu_bct_bwd', dh.data_ptr(), u.data_ptr(), du.data_ptr(), B, C2 // 2, T, _st())
    return du


# ---- squeeze-excite of the ResidualUnit and the FiLM conditioners (csrc/film_se.hip), exact fp32, no atomics

def se_gate_supported(C, inner):
    """True iff the squeeze-excite kernels take the widths (any C >= 1, inner <= 128)"""
    return bool(_lib.query('alm_se_gate_supported', int(C), int(inner)))


def _se_args(u, w1, b1, w2, b2):
    for t in (u, w1, b1, w2, b2):
        _chk(t, F32)
    B, C, T = u.shape
    inner = w1.shape[0]
    assert u.is_contiguous() and all(t.is_contiguous() for t in (w1, b1, w2, b2))
    assert w1.numel() == inner * C and w2.numel() == C * inner and w2.shape[0] == C and b1.numel() == inner and b2.numel() == C
    return B, C, inner, T


def se_gate_fwd(u, w1, b1, w2, b2, *, residual=None):
    """u fp32 [B, C, T] -> u * sigmoid(W2 silu(W1 m + b1) + b2) (+ residual), m = the cumulative mean of u over the CHANNEL axis (the reference's
    SqueezeExcite inside a ResidualUnit); w1 [inner, C(, 1)], w2 [C, inner(, 1)]."""
    B, C, inner, T = _se_args(u, w1, b1, w2, b2)
    if residual is not None:
        _chk(residual, F32)
        assert residual.shape == u.shape and residual.is_contiguous()
    out = _new_like(u)
    _lib.call('alm_se_gate_fwd', u.data_ptr(), _p(residual), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(), B, C, inner, T, _st())
    return out


def se_gate_bwd(g, u, w1, b1, w2, b2):
    """g = dL/dout, u (the forward input) fp32 [B, C, T] -> (du, dW1 like w1, db1, dW2 like w2, db2) of se_gate_fwd (without the residual's gradient);
    everything but u is recomputed, the parameter gradients are summed in a fixed order in a workspace of alm_se_gate_bwd_ws_floats floats."""
    B, C, inner, T = _se_args(u, w1, b1, w2, b2)
    _chk(g, F32)
    assert g.shape == u.shape and g.is_contiguous()
    n = _lib.query('alm_se_gate_bwd_ws_floats', B, C, inner, T)
    if n < 0:
        raise _lib.AlmError('se_gate_bwd: widths outside the kernel envelope (inner <= 128) or a workspace past 2^31 floats')
    ws = _new((n,), dtype=F32, device=u.device)
    du = _new_like(u)
    dw1, db1, dw2, db2 = _new_like(w1), _new_like(b1), _new_like(w2), _new_like(b2)
    _lib.call('alm_se_gate_bwd', g.data_ptr(), u.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), du.data_ptr(), dw1.data_ptr(),
              db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ws.data_ptr(), n, B, C, inner, T, _st())
    return du, dw1, db1, dw2, db2


def _film_args(x, w, b):
    _chk(x, F32), _chk(w, F32), _chk(b, F32)
    C = x.shape[-1]
    assert x.is_contiguous() and w.is_contiguous() and b.is_contiguous() and tuple(w.shape) == (2 * C, 2) and tuple(b.shape) == (2 * C,)
    return x.numel() // C, C


def film_fwd(x, w, b, cond0, cond1):
    """x fp32 [..., C] -> x * gamma + beta, (gamma | beta) = w @ (cond0, cond1) + b with w [2 C, 2], b [2 C] (FiLM.to_cond)"""
    rows, C = _film_args(x, w, b)
    y = _new_like(x)
    _lib.call('alm_film_fwd', x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, C, float(cond0), float(cond1), _st())
    return y


def film_bwd(g, x, w, b, cond0, cond1):
    """(dx, dW [2 C, 2], db [2 C]) of film_fwd; the column sums per row chunk in a workspace of alm_film_bwd_ws_floats floats, added in chunk order"""
    rows, C = _film_args(x, w, b)
    _chk(g, F32)
    assert g.shape == x.shape and g.is_contiguous()
    n = _lib.query('alm_film_bwd_ws_floats', rows, C)
    if n < 0:
        raise _lib.AlmError('film_bwd: the partial-sum workspace exceeds 2^31 floats')
    ws = _new((n,), dtype=F32, device=x.device)
    dx, dw, db = _new_like(x), _new_like(w), _new_like(b)
    _lib.call('alm_film_bwd', g.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), n, rows, C,
              float(cond0), float(cond1), _st())
    return dx, dw, db


# ---- residual finite scalar quantization (csrc/fsq.hip), fp32, no atomics.  One call serves one group: x / out / g / dx are [M, dim_g] views with unit
# element stride (a column slice of a wider matrix is fine); weights = (W_in [d, dim_g], b_in [d], W_out [dim_g, d], b_out [dim_g]) or None (identity)

# The three places where the FSQ paper (arXiv 2309.15505, Appendix A) and vector-quantize-pytorch's FSQ differ; tests/fsq_restated.py names the same
# three, and a check against the installed package is a change of these lines.
FSQ_EPS = 1e-3
FSQ_HALF_L_SIGN = +1                   # half_l = (L - 1) * (1 + FSQ_HALF_L_SIGN * FSQ_EPS) / 2
FSQ_SHIFT_FORM = 'atanh'               # shift = atanh(offset / half_l)   ('tan': the paper's listing)

FSQ_MAX_LEVELS, FSQ_MAX_DIM, FSQ_MAX_QUANTIZERS = 8, 1024, 32
_FSQ_ROWS = dict(half_l=0, offset=1, shift=2, inv_half_w=3, half_w=4, basis=5, levels=6)


def fsq_constants(levels, num_quantizers):
    """the kernels' constant table, fp32 [56 + 16 Q] on the CPU: 7 rows of 8 (half_l, offset, shift, 1 / half_w, half_w, basis, levels; entry j < d
    used, the rest 1) then scale [Q, 8] = (L - 1) ** -q and 1 / scale [Q, 8].  Computed in float64 and rounded once."""
    levels = [int(l) for l in levels]
    d, Q = len(levels), int(num_quantizers)
    assert 1 <= d <= FSQ_MAX_LEVELS and 1 <= Q <= FSQ_MAX_QUANTIZERS and all(l >= 2 for l in levels)
    L = torch.tensor(levels, dtype=torch.float64)
    half_l = (L - 1) * (1 + FSQ_HALF_L_SIGN * FSQ_EPS) / 2
    offset = torch.where(L % 2 == 0, 0.5, 0.).to(torch.float64)
    shift = torch.atanh(offset / half_l) if FSQ_SHIFT_FORM == 'atanh' else torch.tan(offset / half_l)
    half_w = torch.floor(L / 2)
    basis = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), L[:-1]]), dim=0)
    head = torch.ones(7, 8, dtype=torch.float64)
    for name, v in (('half_l', half_l), ('offset', offset), ('shift', shift), ('inv_half_w', 1 / half_w), ('half_w', half_w), ('basis', basis),
                    ('levels', L)):
        head[_FSQ_ROWS[name], :d] = v
    scale = torch.ones(Q, 8, dtype=torch.float64)
    scale[:, :d] = (L - 1)[None, :] ** -torch.arange(Q, dtype=torch.float64)[:, None]
    table = torch.cat([head.reshape(-1), scale.reshape(-1), (1 / scale).reshape(-1)]).to(F32)
    assert table.numel() == _lib.query('alm_fsq_consts_floats', Q)
    return table


def _proj_quant_args(mat, weights, d, Q, consts=None):
    """(M, dim_g, the four weights or four None) of one group's call of the FSQ / LFQ kernels; mat: its [M, dim_g] view; consts: FSQ's table"""
    _chk(mat, F32)
    if consts is not None:
        _chk(consts, F32)
        assert consts.is_contiguous() and consts.numel() == 56 + 16 * Q
    M, dim_g = mat.shape
    assert mat.stride(1) == 1 and d >= 1 and Q >= 1
    if weights is None:
        assert dim_g == d, 'the identity case needs dim_g == the projected width'
        return M, dim_g, (None,) * 4
    w_in, b_in, w_out, b_out = weights
    for t in weights:
        _chk(t, F32)
        assert t.is_contiguous()
    assert tuple(w_in.shape) == (d, dim_g) and tuple(b_in.shape) == (d,) and tuple(w_out.shape) == (dim_g, d) and tuple(b_out.shape) == (dim_g,)
    return M, dim_g, tuple(weights)


def fsq_fwd(x, weights, consts, d, Q, k, idx_out, out, save_z=False):
    """x [M, dim_g] view -> idx_out int64 [M, Q] view (-1 past layer k) and out [M, dim_g] view, both written in place; returns z float64 [M, d] (the
    projected input in the precision the chain runs in, what fsq_bwd needs) with save_z, else None (alm_fsq_fwd)"""
    M, dim_g, (w_in, b_in, w_out, b_out) = _proj_quant_args(x, weights, d, Q, consts)
    _chk(out, F32), _chk(idx_out, torch.int64)
    assert tuple(out.shape) == (M, dim_g) and out.stride(1) == 1 and tuple(idx_out.shape) == (M, Q) and idx_out.stride(1) == 1
    z = _new((M, d), dtype=torch.float64, device=x.device) if save_z else None
    _lib.call('alm_fsq_fwd', x.data_ptr(), x.stride(0), _p(w_in), _p(b_in), _p(w_out), _p(b_out), consts.data_ptr(), idx_out.data_ptr(), idx_out.stride(0),
              out.data_ptr(), out.stride(0), _p(z), M, dim_g, d, Q, int(k), _st())
    return z


def fsq_decode(idx, weights, consts, d, Q, out):
    """idx int64 [M, q <= Q] view (negative = no code) -> out [M, dim_g] view, written in place (alm_fsq_decode)"""
    M, dim_g, (_, _, w_out, b_out) = _proj_quant_args(out, weights, d, Q, consts)
    _chk(idx, torch.int64)
    assert idx.dim() == 2 and idx.shape[0] == M and 1 <= idx.shape[1] <= Q and idx.stride(1) == 1
    _lib.call('alm_fsq_decode', idx.data_ptr(), idx.stride(0), _p(w_out), _p(b_out), consts.data_ptr(), out.data_ptr(), out.stride(0), M, dim_g, d, Q,
              idx.shape[1], _st())
    return out


def fsq_bwd(g, x, z, weights, consts, d, Q, k, dx):
    """g = dL/dout, x [M, dim_g] views, z [M, d] from fsq_fwd (None in the identity case) -> dx view written in place; returns (dW_in, db_in, dW_out,
    db_out), or () in the identity case.  The parameter gradients are per-row-chunk partials in a workspace of alm_fsq_bwd_ws_floats floats, added in
    chunk order by a second launch."""
    M, dim_g, (w_in, _, w_out, _) = _proj_quant_args(x, weights, d, Q, consts)
    _chk(g, F32), _chk(dx, F32)
    assert tuple(g.shape) == (M, dim_g) and g.stride(1) == 1 and tuple(dx.shape) == (M, dim_g) and dx.stride(1) == 1
    grads, ws, n = (), None, 0
    if weights is not None:
        _chk(z, torch.float64)
        assert z.is_contiguous() and tuple(z.shape) == (M, d)
        n = _lib.query('alm_fsq_bwd_ws_floats', M, dim_g, d)
        if n < 0:
            raise _lib.AlmError('fsq_bwd: outside the kernel limits or a workspace past 2^31 floats')
        ws = _new((n,), dtype=F32, device=x.device)
        grads = tuple(_new_like(t) for t in weights)
    dw_in, db_in, dw_out, db_out = grads if grads else (None,) * 4
    _lib.call('alm_fsq_bwd', g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), _p(z), _p(w_in), _p(w_out), consts.data_ptr(), dx.data_ptr(),
              dx.stride(0), _p(dw_in), _p(db_in), _p(dw_out), _p(db_out), _p(ws), n, M, dim_g, d, Q, int(k), _st())
    return grads


# ---- residual lookup-free quantization (csrc/lfq.hip), fp32, no atomics.  One call serves one group, laid out like the FSQ calls above; d =
# log2(codebook_size); weights = (W_in [d, dim_g], b_in [d], W_out [dim_g, d], b_out [dim_g]) or None (identity, dim_g == d).  `loss_cfg` =
# (inv_temperature, entropy_loss_weight, commitment_loss_weight, diversity_gamma)
LFQ_MAX_CODEBOOK_BITS, LFQ_MAX_DIM, LFQ_MAX_QUANTIZERS = 10, 1024, 32
LFQ_INV_TEMPERATURE = 100.             # the package's default; not a constructor argument of the reference


def lfq_fwd(x, weights, d, Q, k, idx_out, out, loss_cfg=None, ws=None):
    """x [M, dim_g] view -> idx_out int64 [M, Q] view (-1 past layer k) and out [M, dim_g] view, both written in place.  With loss_cfg (training
    mode) returns (z float64 [M, d], losses fp32 [Q] (0 past k), avg float64 [Q, 2^d] = the mean code distribution per layer: what lfq_bwd needs),
    else (None, None, None).  ws: a float64 workspace of at least alm_lfq_fwd_ws_doubles elements (allocated when None)  (alm_lfq_fwd)"""
    M, dim_g, (w_in, b_in, w_out, b_out) = _proj_quant_args(x, weights, d, Q)
    _chk(out, F32), _chk(idx_out, torch.int64)
    assert tuple(out.shape) == (M, dim_g) and out.stride(1) == 1 and tuple(idx_out.shape) == (M, Q) and idx_out.stride(1) == 1
    z = losses = avg = None
    tau = w_e = w_c = gamma = 0.
    if loss_cfg is not None:
        tau, w_e, w_c, gamma = (float(v) for v in loss_cfg)
        n = _lib.query('alm_lfq_fwd_ws_doubles', M, d, Q)
        if n < 0:
            raise _lib.AlmError('lfq_fwd: outside the kernel limits or a workspace past 2^31 doubles')
        if ws is None:
            ws = _new((n,), dtype=torch.float64, device=x.device)
        _chk(ws, torch.float64)
        assert ws.is_contiguous()
        z = _new((M, d), dtype=torch.float64, device=x.device)
        losses = _new((Q,), dtype=F32, device=x.device)
        avg = _new((Q, 1 << d), dtype=torch.float64, device=x.device)
    _lib.call('alm_lfq_fwd', x.data_ptr(), x.stride(0), _p(w_in), _p(b_in), _p(w_out), _p(b_out), idx_out.data_ptr(), idx_out.stride(0), out.data_ptr(),
              out.stride(0), _p(z), _p(losses), _p(avg), _p(ws) if loss_cfg is not None else None, ws.numel() if loss_cfg is not None else 0, M, dim_g, d,
              Q, int(k), tau, w_e, w_c, gamma, _st())
    return z, losses, avg


def lfq_decode(idx, weights, d, Q, out):
    """idx int64 [M, q <= Q] view (negative = no code) -> out [M, dim_g] view, written in place (alm_lfq_decode)"""
    M, dim_g, (_, _, w_out, b_out) = _proj_quant_args(out, weights, d, Q)
    _chk(idx, torch.int64)
    assert idx.dim() == 2 and idx.shape[0] == M and 1 <= idx.shape[1] <= Q and idx.stride(1) == 1
    _lib.call('alm_lfq_decode', idx.data_ptr(), idx.stride(0), _p(w_out), _p(b_out), out.data_ptr(), out.stride(0), M, dim_g, d, Q, idx.shape[1], _st())
    return out


def lfq_bwd(g, g_loss, x, z, avg, weights, d, Q, k, dx, loss_cfg, ws=None):
    """g = dL/dout [M, dim_g] view, g_loss = dL/dlosses fp32 [Q] or None, x view, (z, avg) from lfq_fwd -> dx view written in place; returns (dW_in,
    db_in, dW_out, db_out), or () in the identity case.  ws: an fp32 workspace of at least alm_lfq_bwd_ws_floats elements (allocated when None)"""
    M, dim_g, (w_in, _, w_out, _) = _proj_quant_args(x, weights, d, Q)
    _chk(g, F32), _chk(dx, F32), _chk(z, torch.float64)
    assert tuple(g.shape) == (M, dim_g) and g.stride(1) == 1 and tuple(dx.shape) == (M, dim_g) and dx.stride(1) == 1
    assert z.is_contiguous() and tuple(z.shape) == (M, d)
    tau, w_e, w_c, gamma = (float(v) for v in loss_cfg)
    if g_loss is not None:
        _chk(g_loss, F32), _chk(avg, torch.float64)
        assert g_loss.is_contiguous() and tuple(g_loss.shape) == (Q,) and avg.is_contiguous() and tuple(avg.shape) == (Q, 1 << d)
    n = _lib.query('alm_lfq_bwd_ws_floats', M, dim_g, d, Q)
    if n < 0:
        raise _lib.AlmError('lfq_bwd: outside the kernel limits or a workspace past 2^31 floats')
    if ws is None:
        ws = _new((n,), dtype=F32, device=x.device)
    _chk(ws, F32)
    assert ws.is_contiguous()
    grads = tuple(_new_like(t) for t in weights) if weights is not None else ()
    dw_in, db_in, dw_out, db_out = grads if grads else (None,) * 4
    _lib.call('alm_lfq_bwd', g.data_ptr(), g.stride(0), _p(g_loss), x.data_ptr(), x.stride(0), z.data_ptr(), _p(avg) if g_loss is not None else None,
              _p(w_in), _p(w_out), dx.data_ptr(), dx.stride(0), _p(dw_in), _p(db_in), _p(dw_out), _p(db_out), ws.data_ptr(), ws.numel(), M, dim_g, d, Q,
              int(k), tau, w_e, w_c, gamma, _st())
    return grads


# ---- gate-loop layer of SoundStream(use_gate_loop_layers=True) (csrc/gate_loop.hip), exact fp32, no atomics; codec layout [B, C, T]

GATE_LOOP_CHUNK = 4096                 # steps one workgroup scans (alm_gate_loop_chunk): longer rows take the three-launch form


def _gl_dims(x):
    _chk(x, F32)
    assert x.dim() == 3 and x.is_contiguous()
    return x.shape


def _gl_scan_ws(B, C, T, device):
    n = _lib.query('alm_gate_loop_scan_ws_floats', B, C, T)
    if n < 0:
        raise _lib.AlmError('gate_loop scan: B * C * ceil(T / GATE_LOOP_CHUNK) exceeds the kernels\' limit (2^31 / 3)')
    return _new((n,), dtype=F32, device=device) if n else None


def gate_loop_norm_fwd(x, gamma):
    """x fp32 [B, C, T], gamma [C] -> x * r * gamma, r = sqrt(C) / max(||x[b, :, t]||, 1e-12): RMSNorm over the channel axis"""
    B, C, T = _gl_dims(x)
    _chk(gamma, F32)
    assert gamma.is_contiguous() and tuple(gamma.shape) == (C,)
    xn = _new_like(x)
    _lib.call('alm_gate_loop_norm_fwd', x.data_ptr(), gamma.data_ptr(), xn.data_ptr(), B, C, T, _st())
    return xn


def gate_loop_scan_fwd(z, x=None):
    """z fp32 [B, 3 C, T] (rows q | kv | a), x [B, C, T] -> q * h + 2 x with h[t] = sigmoid(a[t]) h[t-1] + kv[t], h[0] = kv[0]; x=None -> h itself"""
    B, C3, T = _gl_dims(z)
    assert C3 % 3 == 0
    C = C3 // 3
    if x is not None:
        assert tuple(_gl_dims(x)) == (B, C, T)
    out = _new((B, C, T), dtype=F32, device=z.device)
    ws = _gl_scan_ws(B, C, T, z.device)
    _lib.call('alm_gate_loop_scan_fwd', z.data_ptr(), _p(x), out.data_ptr(), _p(ws), 0 if ws is None else ws.numel(), B, C, T, int(x is None), _st())
    return out


def gate_loop_scan_bwd(g, z, h):
    """g = dL/dout [B, C, T], z [B, 3 C, T], h = gate_loop_scan_fwd(z) -> dz [B, 3 C, T] (dq | dkv | da rows; da is exactly 0 at t = 0); the 2 g of
    the two skips is left to gate_loop_norm_bwd"""
    B, C, T = _gl_dims(g)
    assert tuple(_gl_dims(z)) == (B, 3 * C, T) and tuple(_gl_dims(h)) == (B, C, T)
    dz = _new_like(z)
    ws = _gl_scan_ws(B, C, T, z.device)
    _lib.call('alm_gate_loop_scan_bwd', g.data_ptr(), z.data_ptr(), h.data_ptr(), dz.data_ptr(), _p(ws), 0 if ws is None else ws.numel(), B, C, T, _st())
    return dz


def gate_loop_norm_bwd(dxn, x, gamma, g):
    """dxn = dL/d(gate_loop_norm_fwd(x, gamma)), g = dL/dout of the block -> (dx [B, C, T] including the 2 g of the two skips, dgamma [C]); dgamma's
    per-block partials in a workspace of alm_gate_loop_norm_bwd_ws_floats floats, added in block order"""
    B, C, T = _gl_dims(x)
    _chk(gamma, F32)
    assert tuple(_gl_dims(dxn)) == (B, C, T) and tuple(_gl_dims(g)) == (B, C, T) and gamma.is_contiguous() and tuple(gamma.shape) == (C,)
    n = _lib.query('alm_gate_loop_norm_bwd_ws_floats', B, C, T)
    if n < 0:
        raise _lib.AlmError('gate_loop_norm_bwd: the partial-sum workspace exceeds 2^31 floats')
    ws = _new((n,), dtype=F32, device=x.device)
    dx, dgamma = _new_like(x), _new_like(gamma)
    _lib.call('alm_gate_loop_norm_bwd', dxn.data_ptr(), x.data_ptr(), gamma.data_ptr(), g.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), ws.data_ptr(), n,
              B, C, T, _st())
    return dx, dgamma


# ---- HuBERT feature model (csrc/hubert.hip; conv1d_valid and mha_attn are the shared fp32 kernels of csrc/dense_f32.hip) ----
def hubert_conv0_stats(wave, w, stride, eps=1e-5):
    """wave fp32 [B, Tin] (unit element stride), w fp32 [C, k] -> stats fp32 [B, C, 2] = (mean, rstd) over time of conv1d(wave, w, stride), the
    activation never stored (alm_hubert_conv0_stats: shifted sums per chunk, chunks merged in order)."""
    _chk(wave, F32)
    _chk(w, F32)
    assert wave.dim() == 2 and w.dim() == 2 and w.is_contiguous()
    wave, ld = _rows(wave)
    B, Tin = wave.shape
    C, k = w.shape
    if Tin < k:
        raise _lib.AlmError(f'the wave has {Tin} samples, fewer than the first conv kernel ({k})')
    Tout = (Tin - k) // stride + 1
    part = _new((B, C, _lib.query('alm_hubert_conv0_chunks', Tout), 2), dtype=F32, device=wave.device)
    stats = _new((B, C, 2), dtype=F32, device=wave.device)
    _lib.call('alm_hubert_conv0_stats', wave.data_ptr(), ld, w.data_ptr(), part.data_ptr(), stats.data_ptr(), B, C, Tin, Tout, k, stride, float(eps), _st())
    return stats


def hubert_conv0_apply(wave, w, stats, gamma, beta, stride):
    """-> fp32 [B, C, Tout] = gelu(GroupNorm(C, C)(conv1d(wave, w, stride))) with the statistics of hubert_conv0_stats"""
    _chk(wave, F32)
    _chk(stats, F32)
    wave, ld = _rows(wave)
    B, Tin = wave.shape
    C, k = w.shape
    Tout = (Tin - k) // stride + 1
    assert stats.shape == (B, C, 2) and stats.is_contiguous() and w.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()
    out = _new((B, C, Tout), dtype=F32, device=wave.device)
    _lib.call('alm_hubert_conv0_apply', wave.data_ptr(), ld, w.data_ptr(), stats.data_ptr(), _chk(gamma, F32).data_ptr(), _chk(beta, F32).data_ptr(),
              out.data_ptr(), B, C, Tin, Tout, k, stride, _st())
    return out


def conv1d_valid(x, w, bias=None, *, stride=1, pad=0, groups=1, gelu=False, residual=None, drop_last=0):
    """x fp32 [B, Cin, Tin], w fp32 [Cout, Cin / groups, k] (torch's layout) -> fp32 [B, Cout, Tout], Tout = (Tin + 2 pad - k) // stride + 1 -
    drop_last: (gelu)(conv + bias) + residual on the exact-fp32 matrix core (alm_conv1d_valid)."""
    _chk(x, F32)
    _chk(w, F32)
    B, Cin, Tin = x.shape
    Cout, Cig, k = w.shape
    assert x.is_contiguous() and w.is_contiguous() and Cig * groups == Cin
    Tout = (Tin + 2 * pad - k) // stride + 1 - drop_last
    if Tout <= 0:
        raise _lib.AlmError(f'conv1d_valid: {Tin} input samples give no output (k = {k}, stride = {stride}, pad = {pad})')
    out = _new((B, Cout, Tout), dtype=F32, device=x.device)
    if bias is not None:
        assert _chk(bias, F32).is_contiguous() and bias.shape == (Cout,)
    if residual is not None:
        assert _chk(residual, F32).is_contiguous() and residual.shape == out.shape
    _lib.call('alm_conv1d_valid', x.data_ptr(), w.data_ptr(), _p(bias), _p(residual), out.data_ptr(), B, Cin, Cout, Tin, Tout, k, stride, pad, groups,
              int(gelu), _st())
    return out


def layernorm_bct_split(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm over the channel axis of x fp32 [B, C, T], parallel over channels (alm_layernorm_bct_split)"""
    _chk(x, F32)
    B, C, T = x.shape
    assert x.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous() and gamma.shape == beta.shape == (C,)
    out = _new_like(x)
    _lib.call('alm_layernorm_bct_split', x.data_ptr(), _chk(gamma, F32).data_ptr(), _chk(beta, F32).data_ptr(), out.data_ptr(), B, C, T, float(eps), _st())
    return out


def mha_attn(qkv, heads, scale=None, dim_head=64):
    """qkv fp32 [B, 3 H dh, T] (q | k | v channel blocks) -> fp32 [B, H dh, T]: bidirectional multi-head attention (alm_mha_attn_fwd)"""
    _chk(qkv, F32)
    B, C3, T = qkv.shape
    assert qkv.is_contiguous() and C3 == 3 * heads * dim_head
    out = _new((B, heads * dim_head, T), dtype=F32, device=qkv.device)
    _lib.call('alm_mha_attn_fwd', qkv.data_ptr(), out.data_ptr(), B, heads, T, dim_head, float(dim_head ** -0.5 if scale is None else scale), _st())
    return out


# ---- vq-wav2vec (csrc/vq_wav2vec.hip): GroupNorm over whole (C / G) x T blocks, fp32 [B, C, T], no atomics ----
def vqw2v_group_stats(x, groups, eps=1e-5):
    """x fp32 [B, C, T] contiguous -> stats fp32 [B, groups, 2] = (mean, rstd) of nn.GroupNorm(groups, C) (alm_vqw2v_group_stats: centred sums per
    chunk of 4096 elements, the chunks merged in a fixed order in fp64)"""
    _chk(x, F32)
    assert x.dim() == 3 and x.is_contiguous()
    B, C, T = x.shape
    chunks = _lib.query('alm_vqw2v_group_chunks', C, T, groups)
    if chunks < 0:
        raise _lib.AlmError(f'vqw2v_group_stats: {groups} groups do not divide {C} channels, or C T = {C * T} does not fit 32 bits')
    part = _new((B, groups, chunks, 2), dtype=F32, device=x.device)
    stats = _new((B, groups, 2), dtype=F32, device=x.device)
    _lib.call('alm_vqw2v_group_stats', x.data_ptr(), part.data_ptr(), stats.data_ptr(), B, C, T, groups, float(eps), _st())
    return stats


def _affine(x, stats, gamma, beta):
    B, C, T = x.shape
    _chk(x, F32), _chk(stats, F32), _chk(gamma, F32), _chk(beta, F32)
    assert x.is_contiguous() and stats.is_contiguous() and stats.dim() == 3 and stats.shape[0] == B and stats.shape[2] == 2
    assert gamma.is_contiguous() and beta.is_contiguous() and gamma.shape == beta.shape == (C,)
    return B, C, T, stats.shape[1]


def vqw2v_group_apply(x, stats, gamma, beta, *, relu=False, residual=None, residual_scale=1.0, log_compression=False):
    """IN PLACE: x fp32 [B, C, T] <- gamma (x - mean) rstd + beta with the statistics of vqw2v_group_stats, then ReLU (relu), then
    (x + residual[..., ::r_T // T][..., :T]) * residual_scale (residual fp32 [B, C, r_T]), then log(|x| + 1) (log_compression)"""
    B, C, T, G = _affine(x, stats, gamma, beta)
    r_T = rstep = 0
    if residual is not None:
        assert _chk(residual, F32).is_contiguous() and residual.shape[:2] == (B, C) and residual.shape[2] >= T
        r_T = residual.shape[2]
        rstep = r_T // T
    _lib.call('alm_vqw2v_group_apply', x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _p(residual), B, C, T, G, r_T, rstep,
              float(residual_scale), int(relu), int(log_compression), _st())
    return x


def vqw2v_group_apply_t(x, stats, gamma, beta):
    """x fp32 [B, C, T] -> fp32 [B, T, C] = gamma (x - mean) rstd + beta, stored transposed (alm_vqw2v_group_apply_t)"""
    B, C, T, G = _affine(x, stats, gamma, beta)
    out = _new((B, T, C), dtype=F32, device=x.device)
    _lib.call('alm_vqw2v_group_apply_t', x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B, C, T, G, _st())
    return out


def vqw2v_conv0_stats(wave, w, stride, eps=1e-5):
    """wave fp32 [B, Tin] (unit element stride), w fp32 [C, k] -> stats fp32 [B, 1, 2] = (mean, rstd) of nn.GroupNorm(1, C) over
    conv1d(wave, w, stride), the activation never stored (alm_vqw2v_conv0_stats: the per-chunk partials of hubert_conv0_stats, merged per row)"""
    _chk(wave, F32)
    _chk(w, F32)
    assert wave.dim() == 2 and w.dim() == 2 and w.is_contiguous()
    wave, ld = _rows(wave)
    B, Tin = wave.shape
    C, k = w.shape
    if Tin < k:
        raise _lib.AlmError(f'the wave has {Tin} samples, fewer than the first conv kernel ({k})')
    Tout = (Tin - k) // stride + 1
    part = _new((B, C, _lib.query('alm_hubert_conv0_chunks', Tout), 2), dtype=F32, device=wave.device)
    stats = _new((B, 1, 2), dtype=F32, device=wave.device)
    _lib.call('alm_vqw2v_conv0_stats', wave.data_ptr(), ld, w.data_ptr(), part.data_ptr(), stats.data_ptr(), B, C, Tin, Tout, k, stride, float(eps), _st())
    return stats


def vqw2v_conv0_apply(wave, w, stats, gamma, beta, stride, log_compression=False):
    """-> fp32 [B, C, Tout] = relu(GroupNorm(1, C)(conv1d(wave, w, stride))) with the statistics of vqw2v_conv0_stats (then log(. + 1))"""
    _chk(wave, F32)
    _chk(stats, F32)
    wave, ld = _rows(wave)
    B, Tin = wave.shape
    C, k = w.shape
    Tout = (Tin - k) // stride + 1
    assert stats.shape == (B, 1, 2) and stats.is_contiguous() and w.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()
    assert gamma.shape == beta.shape == (C,)
    out = _new((B, C, Tout), dtype=F32, device=wave.device)
    _lib.call('alm_vqw2v_conv0_apply', wave.data_ptr(), ld, w.data_ptr(), stats.data_ptr(), _chk(gamma, F32).data_ptr(), _chk(beta, F32).data_ptr(),
              out.data_ptr(), B, C, Tin, Tout, k, stride, int(log_compression), _st())
    return out


# ---- T5 text encoder (csrc/t5.hip; t5_attn: csrc/dense_f32.hip): activations fp32 [C, N], N = B * T columns ----
def t5_embed(ids, table):
    """ids int64 [B, T], table fp32 [vocab, D] -> fp32 [D, B * T] (alm_t5_embed).  An id outside the table is embedded as zeros and raises the
    device error word (see device_error_flag), polled like the other embedding lookups."""
    _chk(table, F32)
    if not ids.is_cuda or ids.dtype != torch.int64:
        raise _lib.AlmError('t5_embed: ids must be an int64 tensor on the GPU')
    assert ids.is_contiguous() and table.is_contiguous() and table.dim() == 2
    N, (vocab, D) = ids.numel(), table.shape
    out = _new((D, N), dtype=F32, device=ids.device)
    poll_device_errors(ids.device)
    _lib.call('alm_t5_embed', ids.data_ptr(), table.data_ptr(), out.data_ptr(), N, D, vocab, device_error_flag(ids.device).data_ptr(), _st())
    return out


def t5_rmsnorm(x, weight, eps=1e-6, mask=None, transpose_out=False):
    """T5LayerNorm over the channel axis of x fp32 [C, N]: weight * x * rsqrt(mean(x^2) + eps) -> [C, N], or [N, C] with transpose_out.
    mask uint8 [N]: exact zeros where it is 0 (alm_t5_rmsnorm)."""
    _chk(x, F32)
    C, N = x.shape
    assert x.is_contiguous() and _chk(weight, F32).is_contiguous() and weight.shape == (C,)
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() == N
    out = _new((N, C) if transpose_out else (C, N), dtype=F32, device=x.device)
    _lib.call('alm_t5_rmsnorm', x.data_ptr(), weight.data_ptr(), _p(mask), out.data_ptr(), C, N, float(eps), int(transpose_out), _st())
    return out


def t5_gate(x, gated=True):
    """gated: x fp32 [2 F, N] -> [F, N] = gelu_new(x[:F]) * x[F:]; else x [F, N] -> relu(x) (alm_t5_gate)"""
    _chk(x, F32)
    R, N = x.shape
    assert x.is_contiguous() and (not gated or R % 2 == 0)
    Fdim = R // 2 if gated else R
    out = _new((Fdim, N), dtype=F32, device=x.device)
    _lib.call('alm_t5_gate', x.data_ptr(), out.data_ptr(), Fdim, N, int(gated), _st())
    return out


def t5_attn(qkv, bias, mask, B, heads, dim_head=64):
    """qkv fp32 [3 H dh, B * T], bias fp32 [H, 2 T - 1] (entry j - i + T - 1 for key j, query i), mask uint8 [B, T] | None -> fp32 [H dh, B * T]:
    T5's bidirectional self-attention, no 1 / sqrt(d) scale (alm_t5_attn_fwd)"""
    _chk(qkv, F32)
    _chk(bias, F32)
    C3, N = qkv.shape
    T = N // B
    assert qkv.is_contiguous() and bias.is_contiguous() and C3 == 3 * heads * dim_head and T * B == N and tuple(bias.shape) == (heads, 2 * T - 1)
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() == N
    out = _new((heads * dim_head, N), dtype=F32, device=qkv.device)
    _lib.call('alm_t5_attn_fwd', qkv.data_ptr(), bias.data_ptr(), _p(mask), out.data_ptr(), B, heads, T, dim_head, _st())
    return out


# ------------------------------------------------------------------------------------------------ EnCodec (csrc/encodec.hip)

def conv1d_causal_pre(x, wp, bias, Cout, ksize, *, stride=1, dilation=1, pre_elu=False, elu=False, residual=None, zero_pad=False):
    """conv1d_causal with a pre-activation: act(bias + conv(ELU(x) if pre_elu else x)) (+ residual); x fp32 [B, Cin, T] -> [B, Cout, T // stride]."""
    _chk(x, F32)
    B, Cin, T = x.shape
    assert x.is_contiguous()
    out = _new((B, Cout, (T - stride) // stride + 1), dtype=F32, device=x.device)
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous()
    _lib.call('alm_conv1d_causal_pre', x.data_ptr(), wp.data_ptr(), bias.data_ptr(), _p(residual), out.data_ptr(), B, Cin, Cout, T, ksize, stride,
              dilation, int(pre_elu), int(elu), int(zero_pad), _st())
    return out


def lstm_launches(T, L):
    return _lib.query('alm_lstm_launches', T, L)


def lstm_seq(xproj, w_ih, w_hh, bias, *, skip=None, out_bct=False):
    """nn.LSTM(H, H, L) over time: xproj fp32 [T, B, 4H] (layer 0's input projection, no bias), w_ih / w_hh [L, 4H, H], bias [L, 4H] (b_ih + b_hh)
    -> the last layer's outputs [T, B, H], or with out_bct [B, H, T] (+ skip [T, B, H]).  One launch per step, all from one C call (alm_lstm_seq)."""
    _chk(xproj, F32)
    T, B, H4 = xproj.shape
    L, H = w_hh.shape[0], w_hh.shape[2]
    assert H4 == 4 * H and w_hh.shape == w_ih.shape == (L, 4 * H, H) and bias.shape == (L, 4 * H)
    assert all(_chk(t, F32).is_contiguous() for t in (xproj, w_ih, w_hh, bias))
    hseq = _new((L, T, B, H), dtype=F32, device=xproj.device)
    c = _new((L, B, H), dtype=F32, device=xproj.device)
    out = _new((B, H, T), dtype=F32, device=xproj.device) if out_bct else None
    if skip is not None:
        assert out_bct and _chk(skip, F32).is_contiguous() and skip.shape == (T, B, H)
    _lib.call('alm_lstm_seq', xproj.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), bias.data_ptr(), hseq.data_ptr(), c.data_ptr(), _p(skip), _p(out),
              T, B, H, L, _st())
    return out if out_bct else hseq[L - 1]


# ---- wave discriminators of SoundStream training (csrc/discr.hip), fp32, no atomics

LOSS_HINGE_DISCR, LOSS_HINGE_GEN, LOSS_L1, LOSS_MSE = (_lib.CONSTANTS['ALM_LOSS_' + n] for n in ('HINGE_DISCR', 'HINGE_GEN', 'L1', 'MSE'))


def gconv1d_out_len(Tin, ksize, stride, padding):
    return _lib.query('alm_gconv1d_out_len', Tin, ksize, stride, padding)


def _gconv_dims(x, w, stride, padding, groups):
    B, Cin, Tin = x.shape
    Cout, cig, K = w.shape
    assert Cin % groups == 0 and Cout % groups == 0 and cig == Cin // groups, (x.shape, w.shape, groups)
    Tout = gconv1d_out_len(Tin, K, stride, padding)
    if Tout < 1:
        raise _lib.AlmError(f'gconv1d: the padded input ({Tin} + 2 * {padding}) is shorter than the kernel ({K})')
    return B, Cin, Cout, Tin, K, Tout


def gconv1d(x, w, bias, *, stride=1, padding=0, groups=1, leaky=False):
    """x fp32 [B, Cin, Tin], w fp32 [Cout, Cin / groups, k] (nn.Conv1d layout), bias [Cout] -> act(conv1d(x, w, bias, stride, padding, groups))
    fp32 [B, Cout, Tout]; leaky: LeakyReLU(0.1)."""
    assert all(_chk(t, F32).is_contiguous() for t in (x, w, bias))
    B, Cin, Cout, Tin, K, Tout = _gconv_dims(x, w, stride, padding, groups)
    y = _new((B, Cout, Tout), dtype=F32, device=x.device)
    _lib.call('alm_gconv1d_fwd', x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), B, Cin, Cout, Tin, K, stride, padding, groups, int(leaky), _st())
    return y


def gconv1d_fwd_masked(v, w, y, *, stride=1, padding=0, groups=1):
    """v fp32 [B, Cin, Tin] -> m(y) conv1d(v, w) fp32 [B, Cout, Tout] without a bias, m(y) = 1 where the saved output y > 0 and 0.1 elsewhere (y None:
    no mask): the derivative of gconv1d_dgrad(g, y, w) with respect to g, applied to v"""
    assert all(_chk(t, F32).is_contiguous() for t in (v, w))
    B, Cin, Cout, Tin, K, Tout = _gconv_dims(v, w, stride, padding, groups)
    if y is not None:
        assert _chk(y, F32).shape == (B, Cout, Tout) and y.is_contiguous()
    out = _new((B, Cout, Tout), dtype=F32, device=v.device)
    _lib.call('alm_gconv1d_fwd_masked', v.data_ptr(), w.data_ptr(), _p(y), out.data_ptr(), B, Cin, Cout, Tin, K, stride, padding, groups, _st())
    return out


def gconv1d_dgrad(g, y, w, Cin, Tin, *, stride=1, padding=0, groups=1):
    """g fp32 [B, Cout, Tout] = dL/dout (times LeakyReLU'(.) taken from the saved output y when y is given) -> dL/dx fp32 [B, Cin, Tin] of gconv1d"""
    assert all(_chk(t, F32).is_contiguous() for t in (g, w))
    B, Cout, Tout = g.shape
    K = w.shape[2]
    assert w.shape[0] == Cout and Tout == gconv1d_out_len(Tin, K, stride, padding)
    if y is not None:
        assert _chk(y, F32).shape == g.shape and y.is_contiguous()
    dx = _new((B, Cin, Tin), dtype=F32, device=g.device)
    _lib.call('alm_gconv1d_dgrad', g.data_ptr(), _p(y), w.data_ptr(), dx.data_ptr(), B, Cin, Cout, Tin, K, stride, padding, groups, _st())
    return dx


def gconv1d_wgrad(g, y, x, ksize, *, stride=1, padding=0, groups=1):
    """g fp32 [B, Cout, Tout] (times LeakyReLU'(.) from y when given), x fp32 [B, Cin, Tin] -> (dW fp32 [Cout, Cin / groups, k], db fp32 [Cout]);
    per-split partial sums in a workspace of alm_gconv1d_wgrad_ws_floats floats, added in split order."""
    assert all(_chk(t, F32).is_contiguous() for t in (g, x))
    B, Cout, Tout = g.shape
    _, Cin, Tin = x.shape
    assert x.shape[0] == B and Tout == gconv1d_out_len(Tin, ksize, stride, padding)
    if y is not None:
        assert _chk(y, F32).shape == g.shape and y.is_contiguous()
    n = _lib.query('alm_gconv1d_wgrad_ws_floats', B, Cin, Cout, Tin, ksize, stride, padding, groups)
    if n < 0:
        raise _lib.AlmError('gconv1d_wgrad: shape outside the kernel envelope (tile / workspace limits)')
    ws = _new((n,), dtype=F32, device=g.device)
    dw = _new((Cout, Cin // groups, ksize), dtype=F32, device=g.device)
    db = _new((Cout,), dtype=F32, device=g.device)
    _lib.call('alm_gconv1d_wgrad', g.data_ptr(), _p(y), x.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), n, B, Cin, Cout, Tin, ksize, stride,
              padding, groups, _st())
    return dw, db


def avgpool1d_out_len(T, f):
    return _lib.query('alm_avgpool1d_out_len', T, f)


def avgpool1d(x, f):
    """nn.AvgPool1d(2 f, stride=f, padding=f) (padding counts in the divisor) along the last axis of a contiguous fp32 tensor"""
    assert _chk(x, F32).is_contiguous() and f >= 1
    T = x.shape[-1]
    y = _new((*x.shape[:-1], avgpool1d_out_len(T, f)), dtype=F32, device=x.device)
    _lib.call('alm_avgpool1d_fwd', x.data_ptr(), y.data_ptr(), x.numel() // T, T, f, _st())
    return y


def avgpool1d_bwd(g, T, f):
    """adjoint of avgpool1d: g [..., T // f + 1] -> [..., T]"""
    assert _chk(g, F32).is_contiguous() and g.shape[-1] == avgpool1d_out_len(T, f)
    dx = _new((*g.shape[:-1], T), dtype=F32, device=g.device)
    _lib.call('alm_avgpool1d_bwd', g.data_ptr(), dx.data_ptr(), dx.numel() // T, T, f, _st())
    return dx


def loss_mean(mode, a, b=None):
    """0-dim fp32 mean over all elements, summed in a fixed order: LOSS_HINGE_DISCR relu(1 + a) + relu(1 - b) (a fake, b real logits),
    LOSS_HINGE_GEN -a, LOSS_L1 |a - b|, LOSS_MSE (a - b)^2, LOSS_L1_COMPLEX the modulus |a - b| of [..., 2] (re, im) pairs, the mean over complex elements"""
    assert _chk(a, F32).is_contiguous() and (b is None) == (mode == LOSS_HINGE_GEN)
    assert mode != LOSS_L1_COMPLEX or a.shape[-1] == 2
    if b is not None:
        assert _chk(b, F32).is_contiguous() and b.shape == a.shape
    out = _new((), dtype=F32, device=a.device)
    ws = _new((_lib.query('alm_loss_ws_floats'),), dtype=F32, device=a.device)
    _lib.call('alm_loss_mean_fwd', a.data_ptr(), _p(b), out.data_ptr(), ws.data_ptr(), a.numel() // (2 if mode == LOSS_L1_COMPLEX else 1), mode, _st())
    return out


def loss_mean_bwd(mode, a, b, gout, need_a=True, need_b=True):
    """(d/da | None, d/db | None) of loss_mean given the upstream gradient gout (0-dim fp32, read on the device)"""
    assert _chk(gout, F32).numel() == 1
    da = _new_like(a) if need_a else None
    db = _new_like(b) if need_b and b is not None else None
    _lib.call('alm_loss_mean_bwd', a.data_ptr(), _p(b), gout.data_ptr(), _p(da), _p(db), a.numel() // (2 if mode == LOSS_L1_COMPLEX else 1), mode, _st())
    return da, db


def grad_penalty(G, weight=10., center=0.):
    """G fp32 [R, n] -> (weight / R sum_r (|G_r| - center)^2 as a 0-dim fp32, the R row norms), every sum in a fixed order"""
    assert _chk(G, F32).is_contiguous() and G.ndim == 2
    R, n = G.shape
    nws = _lib.query('alm_grad_penalty_ws_floats', R, n)
    if nws < 0:
        raise _lib.AlmError(f'grad_penalty: {R} x {n} is outside the kernel envelope (1 .. 65535 non-empty rows)')
    out = _new((), dtype=F32, device=G.device)
    norms = _new((R,), dtype=F32, device=G.device)
    ws = _new((nws,), dtype=F32, device=G.device)
    _lib.call('alm_grad_penalty_fwd', G.data_ptr(), out.data_ptr(), norms.data_ptr(), ws.data_ptr(), nws, R, n, float(weight), float(center), _st())
    return out, norms


def grad_penalty_bwd(G, norms, gout, weight=10., center=0.):
    """d grad_penalty / dG given the upstream gradient gout (0-dim fp32, read on the device); 0 for a row of norm 0"""
    assert all(_chk(t, F32).is_contiguous() for t in (G, norms)) and G.ndim == 2 and norms.shape == (G.shape[0],) and _chk(gout, F32).numel() == 1
    dG = _new_like(G)
    _lib.call('alm_grad_penalty_bwd', G.data_ptr(), norms.data_ptr(), gout.data_ptr(), dG.data_ptr(), G.shape[0], G.shape[1], float(weight), float(center),
              _st())
    return dG


# ---- ComplexSTFTDiscriminator of SoundStream training (csrc/stft_discr.hip), fp32, no atomics.  Complex tensors travel as fp32 [..., 2] (re, im) pairs.

LOSS_L1_COMPLEX = _lib.CONSTANTS['ALM_LOSS_L1_COMPLEX']
_STFT_BASIS = {}


def stft_frames(n, n_fft, hop_length):
    """frames of torch.stft(center=True) on a clip of n samples; -1 unless n > n_fft / 2 (reflect padding needs it)"""
    return _lib.query('alm_stft_frames', n, n_fft, hop_length)


def stft_basis(n_fft, window, normalized, device, onesided=True):
    """windowed DFT basis fp32 [n_fft, 2 F] on `device`: column 2 f = w[k] cos(2 pi f k / n_fft), 2 f + 1 = -w[k] sin(.); `window` is a CPU tensor of
    win_length <= n_fft values, zero-padded and centred.  Built in float64, rounded once, cached per (n_fft, window values, normalized, device)."""
    w = window.detach().to('cpu', torch.float64).reshape(-1)
    assert 0 < w.numel() <= n_fft, (w.numel(), n_fft)
    key = (n_fft, w.numel(), w.numpy().tobytes(), bool(normalized), bool(onesided), str(device))
    hit = _STFT_BASIS.get(key)
    if hit is None:
        F = n_fft // 2 + 1 if onesided else n_fft
        left = (n_fft - w.numel()) // 2
        wp = torch.zeros(n_fft, dtype=torch.float64)
        wp[left:left + w.numel()] = w
        if normalized:
            wp = wp * float(n_fft) ** -0.5
        k = torch.arange(n_fft, dtype=torch.int64)
        ang = ((k[:, None] * torch.arange(F, dtype=torch.int64)[None, :]) % n_fft).to(torch.float64) * (2. * math.pi / n_fft)
        basis = torch.stack((wp[:, None] * torch.cos(ang), -wp[:, None] * torch.sin(ang)), dim=-1).reshape(n_fft, 2 * F)
        if len(_STFT_BASIS) >= 16:
            _STFT_BASIS.clear()
        hit = _STFT_BASIS[key] = basis.to(F32).to(device)
    return hit


def stft(x, basis, n_fft, hop_length):
    """x fp32 [B, n] -> X fp32 [B, F, T, 2] = view_as_real(torch.stft(x, n_fft, hop_length, window=..., center=True, pad_mode='reflect',
    return_complex=True)), the window (and `normalized`) inside `basis` (stft_basis)"""
    assert _chk(x, F32).is_contiguous() and x.ndim == 2 and _chk(basis, F32).is_contiguous() and basis.shape[0] == n_fft and basis.shape[1] % 2 == 0
    B, n = x.shape
    T, F = stft_frames(n, n_fft, hop_length), basis.shape[1] // 2
    if T < 1:
        raise _lib.AlmError(f'stft: a clip of {n} samples is too short for the reflect padding of n_fft = {n_fft} (needs more than n_fft / 2)')
    X = _new((B, F, T, 2), dtype=F32, device=x.device)
    _lib.call('alm_stft_fwd', x.data_ptr(), basis.data_ptr(), X.data_ptr(), B, n, n_fft, hop_length, F, _st())
    return X


def stft_bwd(dX, basis, n, n_fft, hop_length):
    """dX fp32 [B, F, T, 2] -> dx fp32 [B, n]: the adjoint of stft (transposed product, overlap-add, fold of the reflect padding)"""
    assert _chk(dX, F32).is_contiguous() and dX.ndim == 4 and _chk(basis, F32).is_contiguous()
    B, F, T, _ = dX.shape
    assert basis.shape == (n_fft, 2 * F) and T == stft_frames(n, n_fft, hop_length)
    nws = _lib.query('alm_stft_bwd_ws_floats', B, n, n_fft, hop_length)
    if nws < 0:
        raise _lib.AlmError('stft_bwd: shape outside the kernel envelope')
    ws = _new((nws,), dtype=F32, device=dX.device)
    dx = _new((B, n), dtype=F32, device=dX.device)
    _lib.call('alm_stft_bwd', dX.data_ptr(), basis.data_ptr(), dx.data_ptr(), ws.data_ptr(), nws, B, n, n_fft, hop_length, F, _st())
    return dx


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def cconv2d_out_hw(H, W, kernel_size, stride=1, padding=0):
    """(Ho, Wo) of a zero-padded undilated conv2d, or None when the padded input is smaller than the kernel"""
    (kh, kw), (sh, sw), (ph, pw) = _pair(kernel_size), _pair(stride), _pair(padding)
    ho, wo = ctypes.c_int(0), ctypes.c_int(0)
    if _lib.query('alm_cconv2d_out_hw', H, W, kh, kw, sh, sw, ph, pw, ctypes.byref(ho), ctypes.byref(wo)) != 0:
        return None
    return ho.value, wo.value


def _cconv_dims(xshape, wshape, stride, padding):
    B, Cin, H, W, two = xshape
    Cout, Cin_w, kh, kw, two_w = wshape
    assert two == 2 and two_w == 2 and Cin_w == Cin, (tuple(xshape), tuple(wshape))
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    out = cconv2d_out_hw(H, W, (kh, kw), (sh, sw), (ph, pw))
    if out is None:
        raise _lib.AlmError(f'cconv2d: the padded input ({H} + 2 * {ph}, {W} + 2 * {pw}) is smaller than the kernel ({kh}, {kw})')
    return (B, Cin, Cout, H, W, kh, kw, sh, sw, ph, pw), out


def cconv2d(x, w, bias, *, stride=1, padding=0, residual=None):
    """x fp32 [B, Cin, H, W, 2], w fp32 [Cout, Cin, kh, kw, 2], bias fp32 [Cout, 2] (view_as_real of a complex nn.Conv2d's parameters)
    -> view_as_real(F.conv2d(x, w, bias, stride, padding)) fp32 [B, Cout, Ho, Wo, 2] (+ residual of that shape); bias None: no bias"""
    assert all(_chk(t, F32).is_contiguous() for t in (x, w))
    dims, (Ho, Wo) = _cconv_dims(x.shape, w.shape, stride, padding)
    assert bias is None or (_chk(bias, F32).is_contiguous() and bias.shape == (dims[2], 2))
    y = _new((dims[0], dims[2], Ho, Wo, 2), dtype=F32, device=x.device)
    if residual is not None:
        assert _chk(residual, F32).is_contiguous() and residual.shape == y.shape
    _lib.call('alm_cconv2d_fwd', x.data_ptr(), w.data_ptr(), _p(bias), _p(residual), y.data_ptr(), *dims, _st())
    return y


def cconv2d_dgrad(g, w, H, W, *, stride=1, padding=0):
    """g fp32 [B, Cout, Ho, Wo, 2] = dL/dy -> dL/dx fp32 [B, Cin, H, W, 2] of cconv2d"""
    assert all(_chk(t, F32).is_contiguous() for t in (g, w))
    dims, (Ho, Wo) = _cconv_dims((g.shape[0], w.shape[1], H, W, 2), w.shape, stride, padding)
    assert g.shape == (dims[0], dims[2], Ho, Wo, 2), (tuple(g.shape), dims, Ho, Wo)
    dx = _new((dims[0], dims[1], H, W, 2), dtype=F32, device=g.device)
    _lib.call('alm_cconv2d_dgrad', g.data_ptr(), w.data_ptr(), dx.data_ptr(), *dims, _st())
    return dx


def cconv2d_wgrad(g, x, kernel_size, *, stride=1, padding=0):
    """g fp32 [B, Cout, Ho, Wo, 2], x fp32 [B, Cin, H, W, 2] -> (dW fp32 [Cout, Cin, kh, kw, 2], db fp32 [Cout, 2]); per-split partial sums in a
    workspace of alm_cconv2d_wgrad_ws_floats floats, added in split order."""
    assert all(_chk(t, F32).is_contiguous() for t in (g, x))
    kh, kw = _pair(kernel_size)
    dims, (Ho, Wo) = _cconv_dims(x.shape, (g.shape[1], x.shape[1], kh, kw, 2), stride, padding)
    assert g.shape == (dims[0], dims[2], Ho, Wo, 2), (tuple(g.shape), dims, Ho, Wo)
    n = _lib.query('alm_cconv2d_wgrad_ws_floats', *dims)
    if n < 0:
        raise _lib.AlmError('cconv2d_wgrad: shape outside the kernel envelope (index / workspace limits)')
    ws = _new((n,), dtype=F32, device=g.device)
    dw = _new((dims[2], dims[1], kh, kw, 2), dtype=F32, device=g.device)
    db = _new((dims[2], 2), dtype=F32, device=g.device)
    _lib.call('alm_cconv2d_wgrad', g.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), n, *dims, _st())
    return dw, db


def modrelu(z, b):
    """z fp32 [..., 2], b fp32 scalar ON THE DEVICE (never read by the host) -> relu(|z| + b) z / |z| (relu(b) + 0i at z = 0)"""
    assert _chk(z, F32).is_contiguous() and z.shape[-1] == 2 and _chk(b, F32).numel() == 1
    y = _new_like(z)
    _lib.call('alm_modrelu_fwd', z.data_ptr(), b.data_ptr(), y.data_ptr(), z.numel() // 2, _st())
    return y


def modrelu_bwd(g, z, b, need_dz=True):
    """(dz | None, db 0-dim) of modrelu; db is summed in two fixed-order stages"""
    assert all(_chk(t, F32).is_contiguous() for t in (g, z)) and g.shape == z.shape and _chk(b, F32).numel() == 1
    dz = _new_like(z) if need_dz else None
    db = _new((), dtype=F32, device=z.device)
    ws = _new((_lib.query('alm_modrelu_ws_floats'),), dtype=F32, device=z.device)
    _lib.call('alm_modrelu_bwd', g.data_ptr(), z.data_ptr(), b.data_ptr(), _p(dz), db.data_ptr(), ws.data_ptr(), z.numel() // 2, _st())
    return dz, db


def modrelu_bwd2(g, z, b, v, beta, need_dz=True):
    """modrelu_bwd as a function of (g, z, b) against the cotangents v (of dz; None: zero) and beta (0-dim, of db; read on the device), one launch:
    (d/dg, d/dz | None, d/db 0-dim); d/db is summed in the two fixed-order stages of modrelu_bwd"""
    assert all(_chk(t, F32).is_contiguous() for t in (g, z)) and g.shape == z.shape and z.shape[-1] == 2
    assert _chk(b, F32).numel() == 1 and _chk(beta, F32).numel() == 1
    if v is not None:
        assert _chk(v, F32).is_contiguous() and v.shape == z.shape
    dg = _new_like(z)
    dz = _new_like(z) if need_dz else None
    db = _new((), dtype=F32, device=z.device)
    ws = _new((_lib.query('alm_modrelu_ws_floats'),), dtype=F32, device=z.device)
    _lib.call('alm_modrelu_bwd2', g.data_ptr(), z.data_ptr(), b.data_ptr(), _p(v), beta.data_ptr(), dg.data_ptr(), _p(dz), db.data_ptr(), ws.data_ptr(),
              z.numel() // 2, _st())
    return dg, dz, db


def complex_abs_bwd2(g, z, v, need_dz=True):
    """complex_abs_bwd as a function of (g, z) against the cotangent v of dz: (d/dg = u . v, d/dz = g P v / |z| | None); 0 at z = 0"""
    assert all(_chk(t, F32).is_contiguous() for t in (g, z, v)) and tuple(z.shape) == (*g.shape, 2) and v.shape == z.shape
    dg = _new_like(g)
    dz = _new_like(z) if need_dz else None
    _lib.call('alm_cabs_bwd2', g.data_ptr(), z.data_ptr(), v.data_ptr(), dg.data_ptr(), _p(dz), g.numel(), _st())
    return dg, dz


def complex_abs(z):
    """z fp32 [..., 2] -> |z| fp32 [...]"""
    assert _chk(z, F32).is_contiguous() and z.shape[-1] == 2
    y = _new(tuple(z.shape[:-1]), dtype=F32, device=z.device)
    _lib.call('alm_cabs_fwd', z.data_ptr(), y.data_ptr(), y.numel(), _st())
    return y


def complex_abs_bwd(g, z):
    """g fp32 [...], z fp32 [..., 2] -> g z / |z| (0 at z = 0)"""
    assert all(_chk(t, F32).is_contiguous() for t in (g, z)) and tuple(z.shape) == (*g.shape, 2)
    dz = _new_like(z)
    _lib.call('alm_cabs_bwd', g.data_ptr(), z.data_ptr(), dz.data_ptr(), g.numel(), _st())
    return dz


# ---- multi-spectral mel-spectrogram reconstruction loss of SoundStream training (csrc/mel_loss.hip), fp32, no atomics

def mel_power(x, basis, n_fft, hop_length, k_lo, k_hi, x_from=None):
    """x fp32 [B, n] -> (P fp32 [B, F, T] = |STFT|^2, X): the DFT product of `stft` over the basis rows [k_lo, k_hi) (the window's support; the rows
    outside are zeros) with the power formed in its epilogue.  With x_from given, X fp32 [B - x_from, F, T, 2] is the complex spectrum of the batch
    rows from x_from on (what a backward needs); else None."""
    assert _chk(x, F32).is_contiguous() and x.ndim == 2 and _chk(basis, F32).is_contiguous() and basis.shape[0] == n_fft and basis.shape[1] % 2 == 0
    B, n = x.shape
    T, F = stft_frames(n, n_fft, hop_length), basis.shape[1] // 2
    if T < 1:
        raise _lib.AlmError(f'mel_power: a clip of {n} samples is too short for the reflect padding of n_fft = {n_fft} (needs more than n_fft / 2)')
    P = _new((B, F, T), dtype=F32, device=x.device)
    X = None if x_from is None else _new((B - x_from, F, T, 2), dtype=F32, device=x.device)
    _lib.call('alm_mel_power_fwd', x.data_ptr(), basis.data_ptr(), P.data_ptr(), _p(X), B, B if x_from is None else x_from, n, n_fft, hop_length, F,
              k_lo, k_hi, _st())
    return P, X


def mel_project(P, fb):
    """P fp32 [B, F, T], fb fp32 [F, n_mels] -> mel fp32 [B, n_mels, T] = fb^T P"""
    assert _chk(P, F32).is_contiguous() and P.ndim == 3 and _chk(fb, F32).is_contiguous() and fb.ndim == 2 and fb.shape[0] == P.shape[1]
    B, F, T = P.shape
    mel = _new((B, fb.shape[1], T), dtype=F32, device=P.device)
    _lib.call('alm_mel_project_fwd', P.data_ptr(), fb.data_ptr(), mel.data_ptr(), B, F, T, fb.shape[1], _st())
    return mel


def mel_frame_loss(mel, alpha):
    """mel fp32 [2 Bh, n_mels, T] (first half real, second fake) -> (loss 0-dim = means[0] + alpha means[1], means fp32 [2] = (mean over frames of
    sum_m |Mo - Mr|, mean of norms), norms fp32 [Bh, T] = per frame ||log max(Mo, 1e-20) - log max(Mr, 1e-20)||_2), summed in two fixed-order stages"""
    assert _chk(mel, F32).is_contiguous() and mel.ndim == 3 and mel.shape[0] % 2 == 0
    Bh, n_mels, T = mel.shape[0] // 2, mel.shape[1], mel.shape[2]
    norms = _new((Bh, T), dtype=F32, device=mel.device)
    loss = _new((), dtype=F32, device=mel.device)
    means = _new((2,), dtype=F32, device=mel.device)
    ws = _new((_lib.query('alm_mel_loss_ws_floats'),), dtype=F32, device=mel.device)
    _lib.call('alm_mel_frame_loss_fwd', mel.data_ptr(), norms.data_ptr(), loss.data_ptr(), means.data_ptr(), ws.data_ptr(), Bh, n_mels, T, float(alpha), _st())
    return loss, means, norms


def mel_frame_loss_bwd(mel, norms, gout, alpha):
    """d(gout * loss) / d(fake half of mel) fp32 [Bh, n_mels, T] of mel_frame_loss; gout 0-dim fp32, read on the device"""
    assert _chk(mel, F32).is_contiguous() and _chk(norms, F32).is_contiguous() and _chk(gout, F32).numel() == 1
    Bh, n_mels, T = mel.shape[0] // 2, mel.shape[1], mel.shape[2]
    assert norms.shape == (Bh, T)
    dmel = _new((Bh, n_mels, T), dtype=F32, device=mel.device)
    _lib.call('alm_mel_frame_loss_bwd', mel.data_ptr(), norms.data_ptr(), gout.data_ptr(), dmel.data_ptr(), Bh, n_mels, T, float(alpha), _st())
    return dmel


def mel_power_bwd(dmel, fb, X):
    """dmel fp32 [B, n_mels, T], fb fp32 [F, n_mels], X fp32 [B, F, T, 2] -> dX fp32 [B, F, T, 2] = 2 X (fb dmel), the operand of stft_bwd"""
    assert all(_chk(t, F32).is_contiguous() for t in (dmel, fb, X))
    B, n_mels, T = dmel.shape
    F = fb.shape[0]
    assert fb.shape == (F, n_mels) and X.shape == (B, F, T, 2), (tuple(dmel.shape), tuple(fb.shape), tuple(X.shape))
    dX = _new_like(X)
    _lib.call('alm_mel_power_bwd', dmel.data_ptr(), fb.data_ptr(), X.data_ptr(), dX.data_ptr(), B, F, T, n_mels, _st())
    return dX
