"""The 8-byte LDS reads that the fp32 n = 16384 kernels issue from inline asm (NW_LDS_ASM_READS,
nw_shape.h / nw_fft_dev.h), checked without a GPU.

tests/host/lds_reads_check.cpp includes ninwavelets_amd/csrc/nw_shape.h (the constexpr base and
offset functions the kernels compile) and checks, for every thread, component and batch, that the
(base, offset) pairs address exactly the bytes the C++ indexing reads: the 1 -> 2 image's pairs
and the pass-1 table's batches (every power once, at most 8 per batch); that every offset is a
multiple of 8 below 65536; that the last byte read lies inside the image or the table; and that
each 32-lane ds_read_b64 group covers the 64 banks once.  It is built with
-fsanitize=address,undefined and run as a stand-alone program.

Device-only compiles of nw_fused.hip (nothing runs): the switch values 0, 1 and 2 each compile, and
in the default build the body of the flagship kernel (fp32, n = 16384, cwt, real W rows) holds no
ds_read2_b64, which the build with the switch at 0 does.  (The pass-0 X image keeps the
compiler's ds_read2st64_b64: issuing those one by one measured below the bar and is not built,
DESIGN.md §4 Round 15.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
# nw_fused_kernel<float, 16384, 32, NW_OUT_CWT, REALW = true, WSH = 0>
C4_KERNEL = 'nw_fused_kernelIfLi16384ELi32ELi0ELb1ELi0E'
MERGED = ('ds_read2_b64',)


def test_read_addresses_under_asan(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'lds_reads_check')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'lds_reads_check.cpp'),
                    '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'ok'
    fig = dict(zip(lines[0].split()[::2], map(int, lines[0].split()[1::2])))
    # 2 components x 512 x 16, 512 x 31
    assert fig['reads'] == 2 * 512 * 16 + 512 * 31
    assert fig['max_offset'] < 65536
    assert fig['image_end'] <= fig['image_bytes'] == 32 * 544 * 4
    assert fig['table_end'] == fig['image_bytes'] + fig['table_bytes']


def kernel_body(text, key):
    """The instructions of the one kernel whose symbol contains key."""
    m = re.search(r'^(_Z\S*' + re.escape(key) + r'\S*):.*?^\.Lfunc_end', text, re.M | re.S)
    assert m, key
    return [ln.split(';')[0].strip() for ln in m.group(0).splitlines()[1:]]


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    """nw_fused.hip compiled device-only to assembly with the switch at its default and at 0, 1 and
    2, side by side."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    d = tmp_path_factory.mktemp('lds_reads')
    procs = {}
    for mask in (None, 0, 1, 2):
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++20', '-fno-slp-vectorize', '--cuda-device-only', '-w']
        if mask is not None:
            cmd.append(f'-DNW_LDS_ASM_READS={mask}')
        cmd += ['-S', os.path.join(ROOT, 'ninwavelets_amd', 'csrc', 'nw_fused.hip'), '-o', str(d / f'm{mask}.s')]
        procs[mask] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for mask, p in procs.items():
        _, err = p.communicate(timeout=900)
        out[mask] = (p.returncode, err, d / f'm{mask}.s')
    return out


@pytest.mark.parametrize('mask', [0, 1, 2])
def test_each_switch_value_compiles(builds, mask):
    rc, err, path = builds[mask]
    assert rc == 0, err[-2000:]
    body = kernel_body(path.read_text(), C4_KERNEL)
    ops = {op: sum(ln.startswith(op + ' ') for ln in body) for op in MERGED + ('ds_read_b64',)}
    print(mask, ops)
    if mask == 0:                                  # the compiler's loads: the merged form is there
        assert ops['ds_read2_b64'] == 31 and ops['ds_read_b64'] < 10, ops
    else:                                          # one site alone: the other's merged reads stay
        assert 0 < ops['ds_read2_b64'] < 31, ops


def test_default_build_has_no_merged_reads_in_the_flagship_kernel(builds):
    rc, err, path = builds[None]
    assert rc == 0, err[-2000:]
    body = kernel_body(path.read_text(), C4_KERNEL)
    merged = [ln for ln in body if ln.startswith(tuple(op + ' ' for op in MERGED))]
    assert merged == [], merged[:5]
    # 2 x 16 image pairs, 31 table entries
    assert sum(ln.startswith('ds_read_b64 ') for ln in body) >= 32 + 31
