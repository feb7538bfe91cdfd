"""CPU: the C-ABI shared library builds for gfx950, loads, and exports exactly the symbols include/audiolm_hip.h declares; the ctypes binding
derived from that header (_lib.parse_header) reads every declaration form, refuses what it cannot read, and lays the structs out as the
compiler does.  No compute calls: there is no GPU here."""
import ctypes
import os
import re

import pytest

import audiolm_pytorch_amd  # noqa: F401
from audiolm_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'audiolm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\bint\s+(alm_\w+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


# ---- the parser on synthetic headers ----------------------------------------------------------------------------------------------

SYNTHETIC = """
/* a block comment naming alm_foo( and
   spanning lines: int alm_ghost(int x); */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
#define ALM_DEC 10001      // trailing comment with alm_bar(
#define ALM_HEX 0xFFFE
#define NOT_OURS 7
typedef struct { const void* a; int M, N; float alpha; long long lda, ldb; } AlmAnon;   /* 40 bytes */
typedef struct AlmNamed {
    void* p; const float* q;      /* pointers */
    int a, b; long long n;
    float wd; int step;
} AlmNamed;
int alm_multi(const void* A, float* C,
              int M, long long lda,
              float alpha, void* stream);
int alm_void(void);
int alm_empty();
int alm_mixed(const float* const* parts, int* Ho, const unsigned short* reloc, unsigned long long seed, const char* name,
              const unsigned char* mask, const AlmNamed* jobs, const long long* l0);
// int alm_line_comment(int x);
#ifdef __cplusplus
}
#endif
"""


def test_parser_reads_every_declaration_form():
    P, I, L, F, U, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_char_p
    protos, structs, consts = _lib.parse_header(SYNTHETIC)
    assert protos == {'alm_multi': [P, P, I, L, F, P], 'alm_void': [], 'alm_empty': [], 'alm_mixed': [P, P, P, U, S, P, P, P]}
    assert list(protos) == ['alm_multi', 'alm_void', 'alm_empty', 'alm_mixed']
    assert structs == {'AlmAnon': [('a', P), ('M', I), ('N', I), ('alpha', F), ('lda', L), ('ldb', L)],
                       'AlmNamed': [('p', P), ('q', P), ('a', I), ('b', I), ('n', L), ('wd', F), ('step', I)]}
    assert consts == {'ALM_DEC': 10001, 'ALM_HEX': 0xFFFE}


@pytest.mark.parametrize('decl, named', [
    ('int alm_bad(double x);', 'double x'),                                       # unrecognised parameter type
    ('int alm_bad(int M, unsigned n);', 'unsigned n'),
    ('typedef struct { int a; short b; } AlmBad;', 'short b'),                    # unrecognised field type
    ('float alm_bad(int x);', 'alm_bad'),                                         # return type other than int
    ('const char* alm_bad(void);', 'alm_bad'),
    ('int alm_bad(int (*cb)(int), void* stream);', 'alm_bad'),                    # prototype forms the pattern does not consume
    ('static inline int alm_bad(int x) { return x; }', 'alm_bad'),
    ('int alm_bad(int x)', 'alm_bad'),
    ('typedef struct { int a; struct { int b; } in; } AlmBad;', 'AlmBad'),        # a struct it cannot read is not dropped either
    ('#define ALM_BAD (1 << 4)', 'ALM_BAD'),
])
def test_parser_is_strict(decl, named):
    assert list(_lib.parse_header('int alm_before(int x);\nint alm_after(void);\n')[0]) == ['alm_before', 'alm_after']      # the frame alone parses
    with pytest.raises(ValueError) as e:
        _lib.parse_header('int alm_before(int x);\n' + decl + '\nint alm_after(void);\n')
    assert named in str(e.value), str(e.value)


def test_missing_header_is_an_import_error_naming_the_path(tmp_path, monkeypatch):
    """like a missing library: the binding module itself refuses to import (run here as a stand-in package whose build.HEADER points nowhere)"""
    import importlib.util
    import sys
    import types
    pkg, build = types.ModuleType('_alm_nohdr'), types.ModuleType('_alm_nohdr.build')
    pkg.__path__, build.HEADER = [], str(tmp_path / 'gone' / 'audiolm_hip.h')
    monkeypatch.setitem(sys.modules, '_alm_nohdr', pkg)
    monkeypatch.setitem(sys.modules, '_alm_nohdr.build', build)
    spec = importlib.util.spec_from_file_location('_alm_nohdr._lib', os.path.join(ROOT, 'audiolm-pytorch_amd', '_lib.py'))
    with pytest.raises(ImportError) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert build.HEADER in str(e.value)


# ---- the derived binding against independent ground truth -------------------------------------------------------------------------

def test_pinned_rows():
    """real declarations, written out by hand: what the parser makes of the header's own text (not a second copy of the table)"""
    P, I, L, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong
    pinned = {
        'alm_gemm_bf16_nt': [P, P, P, P, I, I, I, L, L, L, I, I, L, L, L, L, L, L, F, I, I, P],
        'alm_mqa_attn_bwd': [P, L, P, L, P, L, P, P, L, P, P, L, P, L, P, P, L, L, P, I, I, I, I, F, F, U, P, P],
        'alm_hc_param_grads_batched': [P, P, I, P, P, P, P, P, I, I, P],
        'alm_list_op_id': [ctypes.c_char_p],
        'alm_cconv2d_out_hw': [I, I, I, I, I, I, I, I, P, P],
        'alm_gemm_nt_ws_bytes': [],
        'alm_opt_chunk_elems': [],
        'alm_list_run': [P, I, P, P, I, P, I, P, P],
        'alm_hubert_conv0_chunks': [L],
        'alm_grad_penalty_ws_floats': [I, L],
        'alm_resample_sinc': [P, L, P, L, P, I, L, L, L, I, I, I, P],
        'alm_gemm_bf16_tn_grouped': [P, I, P, I, P],
    }
    for name, row in pinned.items():
        assert _lib.SIGNATURES[name] == row, name
    assert set(_lib.SIGNATURES) == set(_declared())                 # an independent pattern finds the same names: no prototype was dropped
    assert _lib.CONSTANTS['ALM_ERR_BAD_ARG'] == 10001 and _lib.CONSTANTS['ALM_ERR_UNSUPPORTED'] == 10002
    assert _lib.CONSTANTS['ALM_LIST_STREAM'] == 0xFFFF and _lib.CONSTANTS['ALM_LOSS_L1_COMPLEX'] == 4


STRUCTS = ('AlmTnJob', 'AlmPackJob', 'AlmOptTensor', 'AlmOptPackJob', 'AlmListEntry')


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof / offsetof / field sizes as the C++ compiler of the library build lays the header's structs out == the generated ctypes classes"""
    import subprocess
    header = os.path.join(ROOT, 'include', 'audiolm_hip.h')
    declared = re.findall(r'\}\s*(\w+)\s*;', re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S))
    assert sorted(declared) == sorted(STRUCTS)                      # every struct of the header is one of the five checked below
    lines = []
    for s in STRUCTS:
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        for f, _ in getattr(_lib, s)._fields_:
            lines.append(f'    printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));')
    src = tmp_path / 'layout.cpp'
    src.write_text(f'#include <cstddef>\n#include <cstdio>\n#include "{header}"\nint main() {{\n' + '\n'.join(lines) + '\n    return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++', '-std=c++17', '-o', str(exe), str(src)], check=True, timeout=300)
    got = dict(line.split(' ', 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines())
    want = {}
    for s in STRUCTS:
        cls = getattr(_lib, s)
        assert issubclass(cls, ctypes.Structure) and len(cls._fields_) >= 4
        want[s] = str(ctypes.sizeof(cls))
        for f, t in cls._fields_:
            want[f'{s}.{f}'] = f'{getattr(cls, f).offset} {ctypes.sizeof(t)}'
    assert got == want
    assert ctypes.sizeof(_lib.AlmTnJob) == 128                      # "16 eight-byte words, no padding" (include/audiolm_hip.h)


def test_library_exports_exactly_the_declared_symbols():
    """both directions: an entry point that is defined but not declared (so never type-checked against a prototype, never bound) is as wrong
    as a declared one that is missing"""
    import shutil
    import subprocess
    nm = shutil.which('nm') or next((p for p in ('/opt/rocm/llvm/bin/llvm-nm', '/opt/rocm/lib/llvm/bin/llvm-nm') if os.path.exists(p)), None)
    assert nm, 'neither binutils nm nor the LLVM nm of ROCm found'
    _lib.load()
    out = subprocess.run([nm, '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True, timeout=60).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith('alm_')}
    declared = set(_lib.SIGNATURES)
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))


def test_size_queries_run_on_host():
    assert _lib.query('alm_hc_coef_width', 4) == 52
    assert _lib.query('alm_hc_partial_width', 4, 1024) == 1024 * 7 + 26
    assert _lib.query('alm_hc_grads_width', 4, 1024) == 1024 * 8 + 26
    assert _lib.query('alm_ln_partial_blocks', 16384) == 512


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from audiolm_pytorch_amd import ops
    with pytest.raises(_lib.AlmError):
        ops.gemm_nt(torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8))


def test_import_fails_loudly_without_the_library(tmp_path):
    """No silent fallback: with the shared library unreachable the package import itself raises (nothing on the product path can run)."""
    import subprocess
    import sys
    env = dict(os.environ, ALM_LIB_PATH=str(tmp_path / 'nowhere.so'), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-c', 'import audiolm_pytorch_amd'], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert 'ImportError' in r.stderr and 'nowhere.so' in r.stderr, r.stderr[-500:]


def test_product_modules_do_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under the package may import it"""
    pkg = os.path.join(ROOT, 'audiolm-pytorch_amd')
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), fn


def test_splitk_workspace_covers_the_hybrid_tail():
    """alm_gemm_bf16_tn_batched's hybrid plan (whole waves of 256 tiles at full K + the last problem's remaining blocks as one deep split-K launch)
    writes slices x M2 x N2 partial floats: alm_gemm_splitk_ws_floats, which sizes the caller's workspace, must cover them for every shape the plan
    accepts (host arithmetic only: no GPU).  The plan is restated here from its definition (csrc/gemm.hip hybrid_plan)."""
    import importlib
    L = importlib.import_module('audiolm_pytorch_amd._lib')

    def tail_floats(M, N, K, nb):
        if M < 256 or N < 256 or K < 4096:
            return 0
        tm, tn = -(-M // 256), -(-N // 256)
        m_major = tm >= tn
        tmaj, Q = (tm, tn) if m_major else (tn, tm)
        P, total = tmaj * nb, tmaj * nb * Q
        if total <= 256:
            return 0
        pa = (total // 256) * 256 // Q
        rem = P - pa
        if pa * Q % 256 or rem <= 0 or rem >= tmaj or rem * Q > 64:
            return 0
        off = (tmaj - rem) * 256
        s = 256 // (rem * Q)
        ksteps = -(-K // 64)
        while s > 1 and ksteps // s < 8:
            s -= 1
        if s < 2:
            return 0
        m2, n2 = (M - off, N) if m_major else (M, N - off)
        return s * m2 * n2
    hit = 0
    for M, N in ((2730, 1024), (1024, 2730), (2736, 1024), (4096, 1024), (1024, 512), (3000, 768), (700, 2050)):
        for K in (4096, 8192, 16384, 131072):
            for nb in (1, 2, 3, 6, 12, 24):
                need = tail_floats(M, N, K, nb)
                got = L.query('alm_gemm_splitk_ws_floats', M, N, K, nb)
                assert got == -1 or got >= need, (M, N, K, nb, got, need)
                hit += need > 0
    assert hit >= 10                                            # the benchmark's dW1 / dW2 shapes (6 and 12 problems) are among them
