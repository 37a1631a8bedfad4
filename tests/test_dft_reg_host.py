"""The register DFT (ninwavelets_amd/csrc/nw_dft_reg.h) on the host, without a GPU.

tests/host/dft_reg_check.cpp is a stand-alone program that includes only that header and runs
every (T, R, NZ) the kernels instantiate -- float, double and the packed pair type f2 (where the
compiler has ext_vector_type), R = 2 .. 32, the pass-0 supports NZ, the plain and the twiddled
entry -- on fixed seeded inputs:
  * against a direct O(R^2) DFT in long double: the rms relative error of the product form must
    not exceed 1.5 x the DIF form's (the form up to round 6) on the same inputs; a wrong
    twiddle, sign or zero-mask is an O(1) error;
  * zero stays zero: with r >= NZ zeroed, idft_br<T, R, NZ> equals idft_br<T, R, R> on the same
    padded input to <= 2 ulp of the output norm.
The same program built with -fsanitize=address,undefined must run clean."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'dft_reg_check.cpp')
INC = os.path.join(ROOT, 'ninwavelets_amd', 'csrc')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')


def host_compiler():
    """clang++ (it has the f2 vector type) where there is one, else g++."""
    for c in ('/opt/rocm/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++')):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('dft_reg')
    exes = {'plain': str(d / 'dft_reg_check'), 'san': str(d / 'dft_reg_check_san')}
    procs = {k: subprocess.Popen([cxx, '-std=c++20', '-O1', *(SAN if k == 'san' else []), '-I', INC, SRC, '-o', exe],
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, exe in exes.items()}
    for k, p in procs.items():
        _, err = p.communicate(timeout=1500)
        assert p.returncode == 0, f'{k}: {err[-3000:]}'
    return exes


def test_error_and_zero_checks(programs):
    r = subprocess.run([programs['plain']], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    ratios = [float(m.group(1)) for m in re.finditer(r'ratio ([0-9.]+|inf)', r.stdout)]
    zeros = [float(m.group(1)) for m in re.finditer(r'= ([0-9.]+|inf) ulp', r.stdout)]
    # 5 radices x (plain supports + twiddled entries) x at least float and double
    assert len(ratios) >= 2 * 5 * 4 and len(zeros) >= 2 * 5 * 2
    assert max(ratios) <= 1.5 and max(zeros) <= 2.0
    assert 'FAIL' not in r.stdout
    tw = [float(m.group(1)) for m in re.finditer(r'^tw-\S+ .*ratio ([0-9.]+)', r.stdout, re.M)]
    print(f'error ratio new / DIF: plain and twiddled {min(ratios):.3f} .. {max(ratios):.3f}, '
          f'twiddled alone {min(tw):.3f} .. {max(tw):.3f}; zero check max {max(zeros):.3f} ulp')


def test_runs_clean_under_sanitizers(programs):
    r = subprocess.run([programs['san'], '50'], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith('ok (0 failures)')
