"""Dumps what every alm_gemm_* plan query answers over a shape sweep, one line per query, for the library ALM_LIB_PATH names (default: the in-tree build).
Host arithmetic only: no GPU, no launch.  A/B of two builds (the decisions must not move): run once per library and per environment, each in a fresh
process (the hooks are read once), and compare the outputs line for line:

    ALM_LIB_PATH=/path/to/parent/libaudiolm_hip.so ALM_GEMM_RING=0 python scripts/gemm_plan_dump.py > a.txt
    ALM_GEMM_RING=0 python scripts/gemm_plan_dump.py > b.txt && cmp a.txt b.txt
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from audiolm_pytorch_amd._lib import AlmTnJob  # noqa: E402  (with ALM_LIB_PATH set the package loads that library: nothing is built)
MN = (1, 64, 127, 128, 129, 255, 256, 257, 300, 512, 1024, 1025, 2730, 2736, 5472, 8192, 16384, 16392, 16448)
KS = (8, 64, 200, 256, 1024, 2736, 4096, 16384, 131072)
NB = (1, 2, 3, 6, 12, 24)


def job_lists():
    """the job lists of tests/test_gpu_gemm_tn_grouped.py (the pointers are never dereferenced)"""
    K = 16384
    yield 'mixed', 1096, [(512, 1024, 2), (128, 1024, 2), (600, 520, 1)]
    yield 'headline', K, [(938, 1024, 1), (1024, 426, 1), (1024, 512, 6), (512, 1024, 6), (128, 1024, 6)]
    yield 'tail', 4096, [(256, 4096, 1)]
    yield 'whole', 128, [(4352, 4096, 1)]
    yield 'with_empty', K, [(938, 1024, 1), (0, 1024, 1), (128, 1024, 6)]


def main():
    lib = ctypes.CDLL(os.environ.get('ALM_LIB_PATH') or os.path.join(HERE, '..', 'audiolm-pytorch_amd', 'libaudiolm_hip.so'))
    out = sys.stdout
    p4, p6 = (ctypes.c_int * 4)(), (ctypes.c_int * 6)()
    for M in MN:
        for N in MN:
            for nb in NB:
                out.write(f'nt_tile_choice {M} {N} {nb}: {lib.alm_gemm_nt_tile_choice(M, N, nb)}\n')
                for K in KS:
                    for ws in (0, 1):
                        lib.alm_gemm_nt_plan(M, N, K, nb, ws, p4)
                        out.write(f'nt_plan {M} {N} {K} {nb} ws={ws}: {list(p4)}\n')
                    kind = lib.alm_gemm_tn_batched_plan(M, N, K, nb, p4)
                    out.write(f'tn_batched_plan {M} {N} {K} {nb}: {kind} {list(p4)}\n')
                    out.write(f'splitk {M} {N} {K} {nb}: slices {lib.alm_gemm_splitk_slices(M, N, K, nb)} tile {lib.alm_gemm_splitk_tile(M, N, K, nb)} '
                              f'ws {lib.alm_gemm_splitk_ws_floats(M, N, K, nb)}\n')
    for name, K, shapes in job_lists():
        jobs = (AlmTnJob * len(shapes))()
        for j, (M, N, nb) in zip(jobs, shapes):
            j.At, j.Bt, j.C, j.M, j.N, j.K, j.nb1, j.nb2, j.alpha = 0x100000, 0x200000, 0x300000, M, N, K, nb, 1, 1.0
            j.lda, j.ldb, j.ldc, j.sA1, j.sB1, j.sC1 = 2736 * 2, 2736, N, K * 2736 * 2, K * 2736, M * N
        for slices in range(0, 34):
            S = lib.alm_gemm_tn_grouped_plan(jobs, len(shapes), slices, p6)
            out.write(f'tn_grouped {name} slices={slices}: {S} {list(p6)} ws {lib.alm_gemm_tn_grouped_ws_floats(jobs, len(shapes), slices)}\n')


if __name__ == '__main__':
    main()
