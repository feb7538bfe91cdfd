"""AlmLdsTable (csrc/launch.hpp): the (kernel, device) -> granted-bytes table behind every large-LDS launch.  CPU only: tests/launch_table_main.cpp is
built with the host compiler under AddressSanitizer + UBSan and run as a child process (per-device keys, per-pointer keys, growth, failed sets, threads)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_table_standalone_under_asan_ubsan(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'launch_table')
    # gcc links the sanitizer runtimes dynamically by default, and a dynamic ASan refuses to start behind any other preloaded library: link them in
    gcc = 'clang' not in subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-pthread',
                    *(['-static-libasan', '-static-libubsan'] if gcc else []),
                    '-I', os.path.join(ROOT, 'audiolm-pytorch_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'launch_table_main.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', (r.returncode, r.stdout, r.stderr)
